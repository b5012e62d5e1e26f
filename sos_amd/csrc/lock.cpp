// lock.cpp -- distributed locks: the generic entries behind shmem_set_lock,
// shmem_clear_lock and shmem_test_lock, and the three exported names themselves.
//
// The lock is SOS's MCS queue lock in SOS's word layout (src/shmem_lock.h; lock_proto.h
// describes the words).  A lock composed on the host from blocking atomics would follow
// SOS's sequence atomic_set -> quiet -> swap -> (mswap) -> wait, a launch and a stream
// completion per step.  Here the whole non-waiting part of each call is ONE launch of
// sosx_lock_step (lock.hip) and ONE completion:
//
//  * set_lock: the ENQUEUE kernel stores own data = 0, swaps `last`@PE 0 and, behind a
//    predecessor, ORs me + 1 into the predecessor's data; sync_system; the host reads the
//    record.  ACQUIRED: done.  QUEUED: wait for SIGNAL in own data.
//  * test_lock: the TRY kernel stores own data = 0 and compare-and-swaps `last` from 0;
//    sync_system; 0 when the old value was 0, else 1.
//  * clear_lock: release_system on the stream (SOS's quiet: every put, atomic and kernel
//    store the PE queued before is complete and visible before the next launch starts),
//    then the RELEASE kernel compare-and-swaps `last` from me + 1 to 0 or, where a
//    successor has linked itself, ORs SIGNAL into the successor's data; sync_system.
//    PENDING (a successor swapped `last` but has not linked itself yet): wait for NEXT in
//    own data, then the HANDOFF kernel.  A release or hand-off zeroes own data, so a lock
//    nobody holds or awaits is zero on every PE again.
//
// A wait NEVER spins on the GPU.  It is signal.cpp's host-driven probe: one launch of
// sosx_sync_snapshot on the library stream copies own data into a pinned word, sync_system
// completes it, the host compares, all under spin_until (hostwait.h): after
// SHMEMX_P2P_TIMEOUT seconds the job ends with sos_lock_expiry_message's text.
//
// Consumer half: after a successful acquire a peer's critical section has ended and its
// bytes may have arrived: after_peer_wait (onesided.cpp), as a returning wait does.
//
// Where the lock is: with several PEs, the device symmetric heap (sos_lock_check); with
// one PE any symmetric memory -- a kernel reaches the host heap and a registered data
// segment through device_view, and a lock in pageable static data
// (SHMEMX_REGISTER_DATA=0) is worked on the host with the same step functions over the
// compiler's __atomic builtins, after completing the stream, as amo.cpp does.
//
// Nothing is allocated inside a lock call: the pinned record and the device table of the
// PEs' heap bases are made at shmem_init and the table is refilled when the device heap is
// mapped (lock_table_build); shmem_finalize releases both (lock_release).
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "hostwait.h"
#include "lock_proto.h"
#include "onesided.h"
#include "runtime.h"
#include "sosx.h"

using namespace sosrt;
using soslock::Result;

namespace {

struct LockState {
    Pinned pinned;               // [Result | probe word]
    uint64_t *table = nullptr;   // device: every PE's heap base as mapped here
    std::vector<uint64_t> bases; // the host's copy
    long steps = 0, probes = 0;
};
constexpr size_t kProbeOff = sizeof(Result);
constexpr size_t kPinnedBytes = 64;

LockState &lk()
{
    static LockState l;
    return l;
}

// Where one call's words are, as a kernel (or, host == true, the CPU) reaches them.
struct Where {
    uint32_t *last, *data;
    uint64_t offset;
    bool host;
};

Where locate(long *lock, const char *fn)
{
    State &s = st();
    LockState &g = lk();
    if (!g.table || g.bases.size() != (size_t)s.n_pes) raise_error("%s: the lock table is not set up", fn);
    Where w = {};
    char *mine = nullptr;
    if (s.dev_heap.contains(lock, sizeof(long))) {
        mine = (char *)lock;
        w.last = (uint32_t *)translate(lock, 0);
    } else {
        // one PE (the checks let nothing else come here): PE 0 is the caller
        mine = device_view(lock, sizeof(long));
        w.host = !mine;
        if (w.host) mine = (char *)lock;
        w.last = (uint32_t *)mine;
    }
    w.data = (uint32_t *)(mine + 4);
    w.offset = (uint64_t)(uintptr_t)w.data - g.bases[(size_t)s.my_pe];  // modulo 2^64
    return w;
}

[[noreturn]] void corrupt(const long *lock, int value, const char *fn)
{
    char msg[256];
    sos_lock_corrupt_message(lock, value, st().n_pes, msg, sizeof(msg));
    raise_error("%s: %s", fn, msg);
}

// one step: on the GPU (launch, completion, record) or on the host
Result step(int kind, const Where &w, long *lock, const char *fn)
{
    State &s = st();
    LockState &g = lk();
    Result r;
    if (w.host) {
        hip_check(sync_system(s.stream), fn);  // what the stream still has queued
        const uint64_t base = g.bases[(size_t)s.my_pe];
        using H = soslock::HostAtomics;
        r = kind == SOSX_LOCK_ENQUEUE   ? soslock::enqueue<H>(w.last, w.data, &base, w.offset, 0, 1)
            : kind == SOSX_LOCK_TRY     ? soslock::try_acquire<H>(w.last, w.data, 0, 1)
            : kind == SOSX_LOCK_RELEASE ? soslock::release<H>(w.last, w.data, &base, w.offset, 0, 1)
                                        : soslock::hand_off<H>(w.data, &base, w.offset, 1, 0);
    } else {
        // the chain reads `last` on PE 0: after the acquire a wait may have left owed
        before_peer_read(default_ctx(), 0, fn);
        // SOS's quiet: the release kernel starts after a system-scope release of the
        // stream's earlier work
        if (kind == SOSX_LOCK_RELEASE) hip_check(release_system(s.stream), fn);
        ++g.steps;
        const int rc = sosx_lock_step(kind, w.last, w.data, g.table, w.offset, s.my_pe, s.n_pes, g.pinned.dev, s.stream);
        if (rc != SOSX_OK) raise_error("%s: lock launch failed (%d)", fn, rc);
        hip_check(sync_system(s.stream), fn);
        memcpy(&r, g.pinned.host, sizeof(r));
    }
    if (r.status == SOSX_LOCK_CORRUPT) corrupt(lock, r.bad, fn);
    return r;
}

// own data half now
uint32_t probe(const Where &w, const char *fn)
{
    LockState &g = lk();
    ++g.probes;
    if (w.host) return __atomic_load_n(w.data, __ATOMIC_ACQUIRE);
    State &s = st();
    const int rc = sosx_sync_snapshot((char *)g.pinned.dev + kProbeOff, w.data, 1, sizeof(uint32_t), s.stream);
    if (rc != SOSX_OK) raise_error("%s: snapshot launch failed (%d)", fn, rc);
    hip_check(sync_system(s.stream), fn);
    uint32_t v;
    memcpy(&v, (char *)g.pinned.host + kProbeOff, sizeof(v));
    return v;
}

// until (own data & mask) != 0; returns the value that ended the wait
uint32_t wait_for(const Where &w, uint32_t mask, uint32_t seen, int awaited, long *lock, const char *fn)
{
    if (seen & mask) return seen;
    spin_until([&] { return ((seen = probe(w, fn)) & mask) != 0; }, ProbeCadence{!w.host},
               [&](double seconds) {
                   char msg[384];
                   sos_lock_expiry_message(fn, lock, awaited, seen, seconds, msg, sizeof(msg));
                   raise_error("%s", msg);
               });
    return seen;
}

}  // namespace

// shmem_init, and again whenever the device heap has been created or mapped: the pinned
// record, and the device table of every PE's heap base as this PE maps it (0 where there
// is none yet; sos_lock_check lets no call use such an entry).
void sosrt::lock_table_build()
{
    State &s = st();
    LockState &g = lk();
    if (!g.pinned.host) {
        g.pinned.reserve(kPinnedBytes, s.stream, "lock", "shmem_init");
        memset(g.pinned.host, 0, kPinnedBytes);
    }
    if (!g.table) hip_check(hipMalloc((void **)&g.table, (size_t)s.n_pes * sizeof(uint64_t)), "hipMalloc(lock table)");
    g.bases.assign((size_t)s.n_pes, 0);
    for (size_t q = 0; q < s.peer_heap.size() && q < g.bases.size(); ++q) g.bases[q] = (uint64_t)(uintptr_t)s.peer_heap[q];
    if (s.stream) hip_check(hipStreamSynchronize(s.stream), "hipStreamSynchronize(lock table)");
    hip_check(hipMemcpy(g.table, g.bases.data(), g.bases.size() * sizeof(uint64_t), hipMemcpyHostToDevice),
              "hipMemcpy(lock table)");
}

void sosrt::lock_release()
{
    LockState &g = lk();
    g.pinned.release();
    if (g.table) (void)hipFree(g.table);
    g = LockState();
}

extern "C" {

const uint64_t *sosx_lock_table(int *entries)
{
    if (entries) *entries = (int)lk().bases.size();
    return lk().table;
}

void sosx_lock_stats(long *steps, long *probes)
{
    if (steps) *steps = lk().steps;
    if (probes) *probes = lk().probes;
}

void sos_api_set_lock(long *lock, const char *fn)
{
    checked(sos_lock_check, sos_lock_op{lock}, fn);
    const Where w = locate(lock, fn);
    const Result r = step(SOSX_LOCK_ENQUEUE, w, lock, fn);
    if (r.status == SOSX_LOCK_QUEUED) wait_for(w, soslock::kSignal, r.data, SOS_LOCK_AWAIT_SIGNAL, lock, fn);
    after_peer_wait(st().stream, fn);  // the consumer half of the hand-off
}

int sos_api_test_lock(long *lock, const char *fn)
{
    checked(sos_lock_check, sos_lock_op{lock}, fn);
    const Where w = locate(lock, fn);
    const Result r = step(SOSX_LOCK_TRY, w, lock, fn);
    if (r.status != SOSX_LOCK_ACQUIRED) return 1;
    after_peer_wait(st().stream, fn);  // the consumer half of the hand-off
    return 0;
}

void sos_api_clear_lock(long *lock, const char *fn)
{
    checked(sos_lock_check, sos_lock_op{lock}, fn);
    const Where w = locate(lock, fn);
    Result r = step(SOSX_LOCK_RELEASE, w, lock, fn);
    // a successor swapped `last` but has not linked itself yet: once NEXT is there, the
    // hand-off step (NEXT is checked there, like every value read from the lock)
    if (r.status != SOSX_LOCK_PENDING) return;
    wait_for(w, soslock::kNextMask, r.data, SOS_LOCK_AWAIT_NEXT, lock, fn);
    r = step(SOSX_LOCK_HANDOFF, w, lock, fn);
    if (r.status != SOSX_LOCK_HANDED) raise_error("%s: lock %p: NEXT was seen and is gone (data 0x%08x)", fn, (void *)lock, r.data);
}

// the exported names: strong pshmem_*, weak shmem_* aliases
void pshmem_set_lock(long *lock) { sos_api_set_lock(lock, "shmem_set_lock"); }
void pshmem_clear_lock(long *lock) { sos_api_clear_lock(lock, "shmem_clear_lock"); }
int pshmem_test_lock(long *lock) { return sos_api_test_lock(lock, "shmem_test_lock"); }
void shmem_set_lock(long *lock) __attribute__((weak, alias("pshmem_set_lock")));
void shmem_clear_lock(long *lock) __attribute__((weak, alias("pshmem_clear_lock")));
int shmem_test_lock(long *lock) __attribute__((weak, alias("pshmem_test_lock")));

}  // extern "C"
