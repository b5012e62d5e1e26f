// signal.cpp -- put with signal, the signal operations and the point-to-point waits and
// tests: the generic entries behind shmem_put_signal[_nbi], shmemx_signal_set / _add,
// shmem_signal_fetch, shmem_signal_wait_until and shmem_<T>_wait_until* / _test*
// (signal_gen.cpp).  Their checks and the comparison are plain functions of data
// (onesided_checks.cpp); the entries raise what those refuse (checked, onesided.cpp).
//
//  * put with signal is FUSED -- one launch of sosx_put_signal (putsignal.hip), which copies
//    and then updates the signal word behind a system-scope release -- when target and
//    sig_addr are in the device heap (this PE's or a mapped peer's), a kernel reaches the
//    source (device_view) and the payload is at most SHMEMX_PUT_SIGNAL_FUSED_MAX bytes.
//    Otherwise it is COMPOSED of the existing pieces in stream order, SOS's own sequence
//    (src/data_c.c4:700-712): sos_api_put(nbi), release_system, sos_api_amo SET / ADD on a
//    uint64.  That also covers pageable sources, the calling PE's host heap and static data,
//    and large payloads (the copy engine).
//  * completion: the blocking form returns after sync_system -- source reusable, signal
//    delivered; the nbi form only enqueues, and quiet / fence / barriers complete it.
//  * shmemx_signal_set / _add are the atomic SET / ADD of amo.cpp on a uint64;
//    shmem_signal_fetch is its blocking FETCH on the calling PE's own word.
//  * a wait NEVER spins on the GPU.  Ivars in device memory are probed: one launch of
//    sosx_sync_snapshot on the library stream (so earlier queued work precedes it) copies
//    them into a pinned buffer, sync_system completes it, sos_sync_eval compares on the
//    host.  Ivars the host can address (host heap, data segment) are read with
//    __atomic_load_n after one sync_system for queued operations of the PE itself.
//    wait_until* repeats probes under spin_until (hostwait.h): after SHMEMX_P2P_TIMEOUT
//    seconds the job ends with a message naming the call, the ivar, the comparison, the
//    wanted value and the last value seen.  test* runs exactly one probe.
//  * consumer half: when a wait returns, or a test returns satisfied, a peer's bytes may
//    have arrived: after_peer_wait (onesided.cpp), as user_barrier does after its
//    rendezvous, so later launches on the stream read the payload fresh.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "hostwait.h"
#include "onesided.h"
#include "runtime.h"
#include "shmemx.h"
#include "sosx.h"

using namespace sosrt;

namespace {

// Payloads up to this many bytes take the fused launch (profiles/signal_latency.txt: the
// fused form's median was below putmem_nbi + fence + atomic_set's by more than the spread
// between repetitions at every size measured, 8 B to 64 MiB; nothing larger was measured).
constexpr size_t kFusedMaxDefault = 64u << 20;

struct SignalState {
    size_t fused_max = kFusedMaxDefault;
    bool fused_read = false;
    Pinned snap;  // the probes' snapshot of the ivars
    long fused_calls = 0, composed_calls = 0, probes = 0;
};

SignalState &sig()
{
    static SignalState s;
    return s;
}

size_t fused_max()
{
    SignalState &g = sig();
    if (!g.fused_read) {
        g.fused_max = env_size("SHMEMX_PUT_SIGNAL_FUSED_MAX", kFusedMaxDefault);
        g.fused_read = true;
    }
    return g.fused_max;
}

const char *cmp_name(int cmp)
{
    static const char *names[] = {"?", "SHMEM_CMP_EQ", "SHMEM_CMP_NE", "SHMEM_CMP_GT", "SHMEM_CMP_GE",
                                  "SHMEM_CMP_LT", "SHMEM_CMP_LE"};
    return cmp >= 1 && cmp <= 6 ? names[cmp] : names[0];
}

long long as_signed(const void *p, size_t i, size_t ts)
{
    const char *q = (const char *)p + i * ts;
    if (ts == 2) { int16_t v; memcpy(&v, q, 2); return v; }
    if (ts == 4) { int32_t v; memcpy(&v, q, 4); return v; }
    int64_t v;
    memcpy(&v, q, 8);
    return v;
}

unsigned long long as_unsigned(const void *p, size_t i, size_t ts)
{
    unsigned long long v = 0;
    memcpy(&v, (const char *)p + i * ts, ts);  // little endian
    return v;
}

// One wait or test: its arguments, where the ivars are, and the last snapshot.
struct Sync {
    void *ivars;
    size_t nelems, ts;
    size_t *indices;
    const int *status;
    int cmp;
    const void *value;
    int vector, kind, is_signed;
    const char *fn;
    bool device = false;
    std::vector<uint64_t> host_words;  // snapshot of host-addressable ivars
    const void *snap = nullptr;
    size_t index = SIZE_MAX, count = 0;

    void setup()
    {
        checked(sos_sync_check, sos_sync_op{ivars, nelems, ts, status, indices, kind, cmp}, fn);
        if (!nelems) return;
        device = is_device_ptr(ivars);
        if (device) {
            size_t cap = 4096;  // in powers of two from a page
            while (cap < nelems * ts) cap *= 2;
            sig().snap.reserve(cap, st().stream, "sync snapshot", fn);
        } else {
            // what the stream still has queued (a signal or put of this PE to itself)
            hip_check(sync_system(st().stream), fn);
            host_words.resize((nelems * ts + 7) / 8);
        }
    }

    // one probe: a fresh snapshot, compared
    bool probe()
    {
        ++sig().probes;
        if (!nelems) {
            index = SIZE_MAX;
            count = 0;
            return true;
        }
        if (device) {
            State &s = st();
            const Pinned &buf = sig().snap;
            const int rc = sosx_sync_snapshot(buf.dev, ivars, nelems, ts, s.stream);
            if (rc != SOSX_OK) raise_error("%s: snapshot launch failed (%d)", fn, rc);
            hip_check(sync_system(s.stream), fn);
            snap = buf.host;
        } else {
            char *out = (char *)host_words.data();
            for (size_t i = 0; i < nelems; ++i) {
                if (ts == 2) { const uint16_t v = __atomic_load_n((const uint16_t *)ivars + i, __ATOMIC_ACQUIRE); memcpy(out + 2 * i, &v, 2); }
                else if (ts == 4) { const uint32_t v = __atomic_load_n((const uint32_t *)ivars + i, __ATOMIC_ACQUIRE); memcpy(out + 4 * i, &v, 4); }
                else { const uint64_t v = __atomic_load_n((const uint64_t *)ivars + i, __ATOMIC_ACQUIRE); memcpy(out + 8 * i, &v, 8); }
            }
            snap = out;
        }
        const int r = sos_sync_eval(snap, nelems, ts, is_signed, status, cmp, value, vector, kind, &index, indices,
                                    &count);
        if (r < 0) raise_error("%s: the comparison cannot be evaluated", fn);
        return r != 0;
    }

    bool masked_out() const
    {
        if (!nelems) return true;
        if (!status) return false;
        for (size_t i = 0; i < nelems; ++i)
            if (!status[i]) return false;
        return true;
    }

    size_t result() const { return kind == SOS_SYNC_ANY ? index : kind == SOS_SYNC_SOME ? count : 0; }

    [[noreturn]] void expired(double seconds)
    {
        // the first unmasked ivar that does not satisfy the comparison
        size_t i = 0;
        for (size_t k = 0; k < nelems; ++k) {
            if (status && status[k]) continue;
            size_t idx, cnt;
            const char *w = (const char *)snap + k * ts;
            const char *v = (const char *)value + (vector ? k : 0) * ts;
            if (sos_sync_eval(w, 1, ts, is_signed, nullptr, cmp, v, 0, SOS_SYNC_ONE, &idx, nullptr, &cnt) == 0) {
                i = k;
                break;
            }
        }
        const size_t vi = vector ? i : 0;
        if (is_signed)
            raise_error("%s: no signal after %.0f s (SHMEMX_P2P_TIMEOUT): ivar %p (element %zu of %zu) %s %lld, "
                        "last value seen %lld", fn, seconds, (void *)((char *)ivars + i * ts), i, nelems,
                        cmp_name(cmp), as_signed(value, vi, ts), as_signed(snap, i, ts));
        raise_error("%s: no signal after %.0f s (SHMEMX_P2P_TIMEOUT): ivar %p (element %zu of %zu) %s %llu, "
                    "last value seen %llu", fn, seconds, (void *)((char *)ivars + i * ts), i, nelems, cmp_name(cmp),
                    as_unsigned(value, vi, ts), as_unsigned(snap, i, ts));
    }
};

// put with signal on context `c` (pe: a world PE).  The fused launch counts arrivals on
// the context's own ticket word: launches that share a ticket must be serial, and two
// contexts' streams are not.
void put_signal_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, uint64_t *sig_addr,
                   uint64_t signal, int sig_op, int pe, int nbi, const char *fn)
{
    State &s = st();
    checked(sos_put_signal_check, sos_put_signal_op{dest, source, sig_addr, nelems, type_size, sig_op, pe}, fn);
    const size_t bytes = nelems * type_size;
    const char *sdev = nullptr;
    const bool fused = bytes <= fused_max() && s.dev_heap.contains(sig_addr, sizeof(uint64_t)) &&
                       (!bytes || (s.dev_heap.contains(dest, bytes) && (sdev = device_view(source, bytes))));
    if (fused) {
        ++sig().fused_calls;
        ++c.enqueued;
        if (!c.is_default && !c.ticket) {
            hip_check(hipMalloc((void **)&c.ticket, sizeof(unsigned)), "hipMalloc(put-signal ticket)");
            hip_check(hipMemsetAsync(c.ticket, 0, sizeof(unsigned), c.stream), "hipMemsetAsync(put-signal ticket)");
        }
        const int rc = sosx_put_signal_on(bytes ? translate(dest, pe) : nullptr, sdev, bytes,
                                          (uint64_t *)translate(sig_addr, pe), signal, sig_op, c.ticket, c.stream);
        if (rc != SOSX_OK) raise_error("%s: put-with-signal launch failed (%d)", fn, rc);
    } else {
        ++sig().composed_calls;
        rma_put_on(c, dest, source, nelems, type_size, pe, 1, fn);
        hip_check(release_system(c), fn);
        amo_on(c, sig_op == SOSX_SIGNAL_ADD ? SOSX_AMO_ADD : SOSX_AMO_SET, sig_addr, &signal, nullptr, nullptr, 0,
               sizeof(uint64_t), 0, pe, 0, fn);
    }
    if (!nbi) hip_check(sync_system(c), fn);
}

void signal_op_on(Ctx &c, uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, const char *fn)
{
    if (sig_op != SOSX_SIGNAL_SET && sig_op != SOSX_SIGNAL_ADD)
        raise_error("%s: Argument \"sig_op\", invalid atomic operation for signal (%d)", fn, sig_op);
    amo_on(c, sig_op == SOSX_SIGNAL_ADD ? SOSX_AMO_ADD : SOSX_AMO_SET, sig_addr, &signal, nullptr, nullptr, 0,
           sizeof(uint64_t), 0, pe, 0, fn);
}

}  // namespace

void sosrt::signal_release()
{
    sig().snap.release();
    sosx_put_signal_release();
}

extern "C" {

size_t sosx_set_put_signal_fused_max(size_t bytes)
{
    const size_t old = fused_max();
    sig().fused_max = bytes;
    return old;
}

void sosx_signal_stats(long *fused, long *composed, long *probes)
{
    if (fused) *fused = sig().fused_calls;
    if (composed) *composed = sig().composed_calls;
    if (probes) *probes = sig().probes;
}

void sos_api_put_signal(void *dest, const void *source, size_t nelems, size_t type_size, uint64_t *sig_addr,
                        uint64_t signal, int sig_op, int pe, int nbi, const char *fn)
{
    put_signal_on(default_ctx(), dest, source, nelems, type_size, sig_addr, signal, sig_op, pe, nbi, fn);
}

void sos_api_ctx_put_signal(shmem_ctx_t ctx, void *dest, const void *source, size_t nelems, size_t type_size,
                            uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, int nbi, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    put_signal_on(c, dest, source, nelems, type_size, sig_addr, signal, sig_op, pe, nbi, fn);
}

void sos_api_signal_op(uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, const char *fn)
{
    signal_op_on(default_ctx(), sig_addr, signal, sig_op, pe, fn);
}

void sos_api_ctx_signal_op(shmem_ctx_t ctx, uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    signal_op_on(c, sig_addr, signal, sig_op, pe, fn);
}

uint64_t sos_api_signal_fetch(const uint64_t *sig_addr, const char *fn)
{
    uint64_t old = 0;
    sos_api_amo(SOSX_AMO_FETCH, (void *)sig_addr, nullptr, nullptr, &old, 1, sizeof(uint64_t), 0, st().my_pe, 0, fn);
    return old;
}

size_t sos_api_wait(void *ivars, size_t nelems, size_t *indices, const int *status, int cmp, const void *value,
                    int vector, int kind, size_t type_size, int is_signed, uint64_t *satisfied, const char *fn)
{
    // the deprecated shmem_<T>_wait: until the ivar differs from value
    Sync w = {ivars, nelems, type_size, indices, status, cmp < 0 ? 2 : cmp, value, vector, kind, is_signed, fn};
    w.setup();
    if (w.masked_out()) return w.result();  // SIZE_MAX for ANY, 0 otherwise: nothing to wait for
    spin_until([&] { return w.probe(); }, ProbeCadence{w.device}, [&](double seconds) { w.expired(seconds); });
    after_peer_wait(st().stream, fn);  // the consumer half of the hand-off
    if (satisfied) *satisfied = as_unsigned(w.snap, 0, type_size);
    return w.result();
}

size_t sos_api_test(void *ivars, size_t nelems, size_t *indices, const int *status, int cmp, const void *value,
                    int vector, int kind, size_t type_size, int is_signed, const char *fn)
{
    Sync t = {ivars, nelems, type_size, indices, status, cmp, value, vector, kind, is_signed, fn};
    t.setup();
    if (t.masked_out()) return kind == SOS_SYNC_ALL ? 1 : t.result();  // as SOS's loops leave it
    const bool ok = t.probe();
    if (ok) after_peer_wait(st().stream, fn);
    if (kind == SOS_SYNC_ONE || kind == SOS_SYNC_ALL) return ok ? 1 : 0;
    return t.result();
}

}  // extern "C"
