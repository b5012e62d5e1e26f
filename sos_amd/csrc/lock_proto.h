// lock_proto.h -- the non-waiting steps of the distributed lock (shmem_set_lock,
// shmem_test_lock, shmem_clear_lock), written once over a small atomics backend.  No HIP
// header: the kernels of lock.hip run these functions over system-scope __hip_atomic_*
// operations, lock.cpp runs them over the compiler's __atomic builtins for a lock only the
// host can address, and tests/lock_proto_harness.cpp runs them between CPU threads.
//
// The lock is SOS's MCS queue lock in SOS's word layout (src/shmem_lock.h): the `long` is
// two 32-bit halves,
//
//   last  (byte 0)  PE id + 1 of the queue's tail; meaningful on PE 0 only (its home)
//   data  (byte 4)  meaningful on every PE: bits 0-30 NEXT, the successor's PE id + 1;
//                   bit 31 SIGNAL, "the lock is yours"
//
// and a free lock is all zero on every PE.  PE q's data half is at table[q] + offset: the
// caller passes every PE's base and the lock's offset, because the step learns which peer
// to touch (the predecessor, the successor) only from the values it reads.  Such a value is
// checked against 1..n_pes BEFORE any address is formed from it; out of range, no peer word
// is touched and the step reports LOCK_CORRUPT with the value.
//
// A step never waits.  Where the algorithm must wait (for SIGNAL after queueing, for NEXT
// when a successor has swapped `last` but not yet linked itself) the step says so in its
// status and the caller probes the PE's own data half.
//
// Backend: a type with static functions over uint32_t words
//   store(p, v)            atomic store of the PE's own word
//   load(p)                atomic load of the PE's own word
//   exchange(p, v)         -> old value
//   cas(p, expect, value)  -> old value (stored if it equalled expect)
//   fetch_or(p, v)         -> old value
// exchange, cas and fetch_or are releases (everything the caller did before is visible to
// whoever reads the new value); the CPU backend's are acquires as well, where the GPU
// caller runs its acquire on the stream after the kernel (lock.cpp).
#pragma once
#include <stdint.h>

#ifndef SOS_LOCK_FN
#define SOS_LOCK_FN inline
#endif

namespace soslock {

constexpr uint32_t kNextMask = 0x7FFFFFFFu;
constexpr uint32_t kSignal = 0x80000000u;

enum Kind : int { LOCK_ENQUEUE = 0, LOCK_TRY = 1, LOCK_RELEASE = 2, LOCK_HANDOFF = 3 };

enum Status : int {
    LOCK_ACQUIRED = 0,  // enqueue / try: the lock is the caller's
    LOCK_QUEUED = 1,    // enqueue: linked behind prev; wait for SIGNAL in own data
    LOCK_BUSY = 2,      // try: somebody holds it; nothing but own data was written
    LOCK_RELEASED = 3,  // release: nobody was queued, `last` is zero again
    LOCK_HANDED = 4,    // release / hand-off: SIGNAL set in the successor's data
    LOCK_PENDING = 5,   // release / hand-off: a successor exists but has not linked itself
                        // yet; wait for NEXT in own data, then run the hand-off step
    LOCK_CORRUPT = 6,   // a value read from the lock is no PE id + 1: nothing more touched
};

// What a step leaves for its caller (the kernel: in a pinned host word).
struct Result {
    int32_t prev;    // the old value of `last`
    uint32_t data;   // own data half as last seen (0 where the step did not look)
    int32_t status;  // Status
    int32_t bad;     // LOCK_CORRUPT: the value that is no PE id + 1
};

SOS_LOCK_FN bool in_queue_range(int32_t v, int n_pes) { return v >= 1 && v <= n_pes; }

SOS_LOCK_FN uint32_t *data_word(const uint64_t *table, uint64_t offset, int pe)
{
    return (uint32_t *)(uintptr_t)(table[pe] + offset);
}

// set_lock up to its wait: own data = 0, swap `last`, link behind the predecessor.
template <class A>
SOS_LOCK_FN Result enqueue(uint32_t *last, uint32_t *my_data, const uint64_t *table, uint64_t offset, int me, int n_pes)
{
    Result r = {0, 0, LOCK_ACQUIRED, 0};
    A::store(my_data, 0u);
    // a release: the zero above is in place before any PE can learn of this one from `last`
    r.prev = (int32_t)A::exchange(last, (uint32_t)(me + 1));
    if (r.prev == 0) return r;
    if (!in_queue_range(r.prev, n_pes)) {
        r.status = LOCK_CORRUPT;
        r.bad = r.prev;
        return r;
    }
    // SOS writes NEXT with a masked swap (mask 0x7FFFFFFF) of me + 1.  One atomic OR of
    // me + 1 leaves the same word: the predecessor zeroed its data before it published
    // itself in `last`, so NEXT is 0 there; exactly one successor -- the one whose swap
    // returned that predecessor -- ever writes it; and the only bit that can change
    // concurrently is 31, which the OR, like the masked swap, preserves.
    A::fetch_or(data_word(table, offset, r.prev - 1), (uint32_t)(me + 1));
    r.data = A::load(my_data);
    r.status = (r.data & kSignal) ? LOCK_ACQUIRED : LOCK_QUEUED;
    return r;
}

// test_lock: own data = 0, `last` from 0 to me + 1 or not at all.
template <class A> SOS_LOCK_FN Result try_acquire(uint32_t *last, uint32_t *my_data, int me, int n_pes)
{
    Result r = {0, 0, LOCK_ACQUIRED, 0};
    A::store(my_data, 0u);
    r.prev = (int32_t)A::cas(last, 0u, (uint32_t)(me + 1));
    if (r.prev == 0) return r;
    r.status = LOCK_BUSY;
    if (!in_queue_range(r.prev, n_pes)) {
        r.status = LOCK_CORRUPT;
        r.bad = r.prev;
    }
    return r;
}

// The hand-off: SIGNAL into the data of the successor named by own data's NEXT, which must
// have linked itself (else LOCK_PENDING and nothing changed).  Own data is zero afterwards:
// the predecessor's SIGNAL and the successor's NEXT have both been consumed, and nobody
// writes the word again before this PE queues anew -- so a lock nobody holds or awaits is
// all zero on every PE, as before its first use.
template <class A>
SOS_LOCK_FN Result hand_off(uint32_t *my_data, const uint64_t *table, uint64_t offset, int n_pes, int32_t prev)
{
    Result r = {prev, A::load(my_data), LOCK_HANDED, 0};
    const int32_t next = (int32_t)(r.data & kNextMask);
    if (next == 0) {
        r.status = LOCK_PENDING;
        return r;
    }
    if (!in_queue_range(next, n_pes)) {
        r.status = LOCK_CORRUPT;
        r.bad = next;
        return r;
    }
    // a release: the critical section's stores are visible before the successor sees SIGNAL
    A::fetch_or(data_word(table, offset, next - 1), kSignal);
    A::store(my_data, 0u);
    return r;
}

// clear_lock after its quiet: `last` from me + 1 to 0 (a release), else the hand-off.
template <class A>
SOS_LOCK_FN Result release(uint32_t *last, uint32_t *my_data, const uint64_t *table, uint64_t offset, int me, int n_pes)
{
    Result r = {0, 0, LOCK_RELEASED, 0};
    r.prev = (int32_t)A::cas(last, (uint32_t)(me + 1), 0u);
    if (r.prev == me + 1) {
        // nobody can have learnt of this PE from `last` any more: drop the SIGNAL it was
        // granted with
        A::store(my_data, 0u);
        return r;
    }
    if (!in_queue_range(r.prev, n_pes)) {  // 0 too: nobody holds this lock
        r.status = LOCK_CORRUPT;
        r.bad = r.prev;
        return r;
    }
    return hand_off<A>(my_data, table, offset, n_pes, r.prev);
}

// The CPU backend (lock.cpp's host path, tests/lock_proto_harness.cpp).
struct HostAtomics {
    static void store(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
    static uint32_t load(uint32_t *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static uint32_t exchange(uint32_t *p, uint32_t v) { return __atomic_exchange_n(p, v, __ATOMIC_ACQ_REL); }
    static uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v)
    {
        __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
        return expect;  // the word's value either way
    }
    static uint32_t fetch_or(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_ACQ_REL); }
};

}  // namespace soslock
