// lock_proto_harness.cpp -- the step functions of sos_amd/csrc/lock_proto.h over the CPU
// backend, as a program of its own (tests/test_lock_proto.py builds it plain, with
// -fsanitize=address,undefined and with -fsanitize=thread).
//
//   lock_proto_harness scripts        deterministic scripts, every word compared after every
//                                     step with a model of the queue written here (a deque
//                                     of PE ids), not taken from the header
//   lock_proto_harness threads P R    P threads, R rounds each of set, counter++ (not
//                                     atomic), clear; the waits are host spins
//
// The P lock words lie in one array with guard words on both sides; every check looks at
// the guards too, so a step that formed an address from a value it should have refused
// shows up as a changed guard (and, under the address sanitizer, as a report).
#include <limits.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <thread>
#include <vector>

#include "lock_proto.h"

using namespace soslock;
using A = HostAtomics;

namespace {

constexpr int kGuard = 8;  // 64-bit guard words on each side
constexpr uint64_t kGuardValue = 0xC0FFEE0DDBA11ull;

int g_checks = 0;

#define FAIL(...)                                   \
    do {                                            \
        fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);               \
        fprintf(stderr, "\n");                      \
        exit(1);                                    \
    } while (0)

// P emulated PEs: PE q's lock word is words[q]; last = low half, data = high half.
struct Arena {
    int P;
    std::vector<uint64_t> mem;
    std::vector<uint64_t> table;
    explicit Arena(int p) : P(p), mem((size_t)(p + 2 * kGuard), 0), table((size_t)p)
    {
        for (int i = 0; i < kGuard; ++i) mem[(size_t)i] = mem[(size_t)(kGuard + p + i)] = kGuardValue;
        for (int q = 0; q < p; ++q) table[(size_t)q] = (uint64_t)(uintptr_t)&mem[(size_t)(kGuard + q)];
    }
    uint32_t *last(int q = 0) { return (uint32_t *)&mem[(size_t)(kGuard + q)]; }
    uint32_t *data(int q) { return last(q) + 1; }
    static constexpr uint64_t offset = 4;
    void guards_intact(const char *what)
    {
        for (int i = 0; i < kGuard; ++i)
            if (mem[(size_t)i] != kGuardValue || mem[(size_t)(kGuard + P + i)] != kGuardValue)
                FAIL("%s: guard word %d changed", what, i);
        ++g_checks;
    }
};

// The model: who is in the queue (front = holder), who has linked itself behind its
// predecessor, and who was granted the lock by a hand-off.
struct Model {
    int P;
    std::deque<int> queue;
    std::vector<bool> linked, signalled;
    explicit Model(int p) : P(p), linked((size_t)p, false), signalled((size_t)p, false) {}
    uint32_t want_last() const { return queue.empty() ? 0u : (uint32_t)(queue.back() + 1); }
    uint32_t want_data(int q) const
    {
        for (size_t i = 0; i < queue.size(); ++i) {
            if (queue[i] != q) continue;
            uint32_t v = signalled[(size_t)q] ? 0x80000000u : 0u;
            if (i + 1 < queue.size() && linked[(size_t)queue[i + 1]]) v |= (uint32_t)(queue[i + 1] + 1);
            return v;
        }
        return 0;  // not queued: zero
    }
    void join(int q, bool link)
    {
        queue.push_back(q);
        linked[(size_t)q] = link;
        signalled[(size_t)q] = false;
    }
    void leave()
    {
        queue.pop_front();
        if (!queue.empty()) signalled[(size_t)queue.front()] = true;
    }
};

void compare(Arena &a, const Model &m, const char *what)
{
    if (*a.last(0) != m.want_last()) FAIL("%s: last = %u, model %u", what, *a.last(0), m.want_last());
    for (int q = 0; q < a.P; ++q) {
        if (q && *a.last(q)) FAIL("%s: PE %d's last half = %u (only PE 0's is ever written)", what, q, *a.last(q));
        if (*a.data(q) != m.want_data(q)) FAIL("%s: PE %d data = 0x%08x, model 0x%08x", what, q, *a.data(q), m.want_data(q));
    }
    a.guards_intact(what);
    ++g_checks;
}

void expect(const Result &r, int status, int prev, const char *what)
{
    if (r.status != status || r.prev != prev) FAIL("%s: status %d prev %d, expected %d %d", what, r.status, r.prev, status, prev);
    ++g_checks;
}

Result do_enqueue(Arena &a, int me) { return enqueue<A>(a.last(), a.data(me), a.table.data(), Arena::offset, me, a.P); }
Result do_try(Arena &a, int me) { return try_acquire<A>(a.last(), a.data(me), me, a.P); }
Result do_release(Arena &a, int me) { return release<A>(a.last(), a.data(me), a.table.data(), Arena::offset, me, a.P); }
Result do_handoff(Arena &a, int me) { return hand_off<A>(a.data(me), a.table.data(), Arena::offset, a.P, 0); }

void script_uncontended()
{
    for (int me = 0; me < 4; ++me) {
        Arena a(4);
        Model m(4);
        compare(a, m, "fresh lock");
        expect(do_enqueue(a, me), LOCK_ACQUIRED, 0, "uncontended enqueue");
        m.join(me, true);
        compare(a, m, "after uncontended enqueue");
        expect(do_release(a, me), LOCK_RELEASED, me + 1, "uncontended release");
        m.leave();
        compare(a, m, "after uncontended release");
        // and through try
        expect(do_try(a, me), LOCK_ACQUIRED, 0, "try on a free lock");
        m.join(me, true);
        compare(a, m, "after try");
        expect(do_release(a, me), LOCK_RELEASED, me + 1, "release after try");
        m.leave();
        compare(a, m, "all zero again");
    }
}

void script_queue_0_2_1()
{
    Arena a(3);
    Model m(3);
    expect(do_enqueue(a, 0), LOCK_ACQUIRED, 0, "PE 0 enqueues");
    m.join(0, true);
    compare(a, m, "0 holds");
    expect(do_enqueue(a, 2), LOCK_QUEUED, 1, "PE 2 enqueues");
    m.join(2, true);
    compare(a, m, "0 holds, 2 waits");
    expect(do_enqueue(a, 1), LOCK_QUEUED, 3, "PE 1 enqueues");
    m.join(1, true);
    compare(a, m, "0 holds, 2 and 1 wait");
    if (*a.data(2) & kSignal) FAIL("PE 2 was signalled early");
    Result r = do_release(a, 0);
    expect(r, LOCK_HANDED, 2, "PE 0 releases");
    if (r.data != 3u) FAIL("PE 0's record holds data 0x%08x, expected NEXT = 3", r.data);
    m.leave();
    compare(a, m, "2 holds, 1 waits");
    if (!(*a.data(2) & kSignal) || (*a.data(1) & kSignal)) FAIL("the hand-off reached the wrong PE");
    expect(do_release(a, 2), LOCK_HANDED, 2, "PE 2 releases");
    m.leave();
    compare(a, m, "1 holds");
    expect(do_release(a, 1), LOCK_RELEASED, 2, "PE 1 releases");
    m.leave();
    compare(a, m, "all zero again");
}

void script_try_on_held()
{
    Arena a(4);
    Model m(4);
    expect(do_enqueue(a, 1), LOCK_ACQUIRED, 0, "PE 1 enqueues");
    m.join(1, true);
    *a.data(3) = 0x1234u;  // stale: try must zero own data, and touch nothing else
    expect(do_try(a, 3), LOCK_BUSY, 2, "try on a held lock");
    compare(a, m, "after the failed try");
    expect(do_try(a, 1), LOCK_BUSY, 2, "try by the holder itself");
    // the holder's own data is zeroed by its try, as SOS does; no successor was linked
    compare(a, m, "after the holder's try");
    expect(do_release(a, 1), LOCK_RELEASED, 2, "PE 1 releases");
    m.leave();
    compare(a, m, "all zero again");
}

void script_pending()
{
    Arena a(4);
    Model m(4);
    expect(do_enqueue(a, 3), LOCK_ACQUIRED, 0, "PE 3 enqueues");
    m.join(3, true);
    // PE 1's enqueue, stopped between its swap and its link
    A::store(a.data(1), 0u);
    if (A::exchange(a.last(), 2u) != 4u) FAIL("the split enqueue's swap");
    m.join(1, false);
    compare(a, m, "3 holds, 1 swapped but not linked");
    const std::vector<uint64_t> before = a.mem;
    Result r = do_release(a, 3);
    expect(r, LOCK_PENDING, 2, "release before the link");
    if (a.mem != before) FAIL("a PENDING release changed a word");
    expect(do_handoff(a, 3), LOCK_PENDING, 0, "hand-off before the link");
    if (a.mem != before) FAIL("a PENDING hand-off changed a word");
    // the rest of PE 1's enqueue
    A::fetch_or(a.data(3), 2u);
    m.linked[1] = true;
    compare(a, m, "3 holds, 1 linked");
    r = do_handoff(a, 3);
    expect(r, LOCK_HANDED, 0, "the later hand-off");
    if (r.data != 2u) FAIL("the hand-off's record holds data 0x%08x", r.data);
    m.leave();
    compare(a, m, "1 holds");
    expect(do_release(a, 1), LOCK_RELEASED, 2, "PE 1 releases");
    m.leave();
    compare(a, m, "all zero again");
}

void script_corrupt()
{
    const int P = 4;
    const int32_t values[] = {0, P, P + 1, INT_MAX, -1, INT_MIN, -P};
    for (int32_t v : values) {
        const bool in_range = v >= 1 && v <= P;
        // a garbage `last` met by enqueue: 0 is a free lock, 1..P a predecessor
        {
            Arena a(P);
            *a.last() = (uint32_t)v;
            const std::vector<uint64_t> before = a.mem;
            const Result r = do_enqueue(a, 1);
            if (v == 0) expect(r, LOCK_ACQUIRED, 0, "enqueue on last = 0");
            else if (in_range) expect(r, LOCK_QUEUED, v, "enqueue behind a valid predecessor");
            else {
                expect(r, LOCK_CORRUPT, v, "enqueue on a garbage last");
                if (r.bad != v) FAIL("enqueue: bad = %d, expected %d", r.bad, v);
                // only `last` (the swap happened) and own data (zeroed) may differ
                for (size_t i = 0; i < a.mem.size(); ++i)
                    if (i != (size_t)kGuard && i != (size_t)(kGuard + 1) && a.mem[i] != before[i])
                        FAIL("enqueue on last = %d wrote word %zu", v, i);
                if (*a.data(0) != 0) FAIL("enqueue on last = %d touched PE 0's data", v);
            }
            a.guards_intact("enqueue on a garbage last");
        }
        // ... by try: no address is formed, but a garbage lock is reported
        {
            Arena a(P);
            *a.last() = (uint32_t)v;
            const Result r = do_try(a, 2);
            if (v == 0) expect(r, LOCK_ACQUIRED, 0, "try on last = 0");
            else if (in_range) expect(r, LOCK_BUSY, v, "try on a held lock");
            else expect(r, LOCK_CORRUPT, v, "try on a garbage last");
            if (v != 0 && *a.last() != (uint32_t)v) FAIL("a failed try changed last");
            a.guards_intact("try on a garbage last");
        }
        // ... by release: me + 1 releases, 1..P is a successor's, anything else is no lock
        {
            Arena a(P);
            *a.last() = (uint32_t)v;
            const std::vector<uint64_t> before = a.mem;
            const Result r = do_release(a, 1);  // me + 1 == 2
            if (v == 2) expect(r, LOCK_RELEASED, 2, "release by the tail");
            else if (in_range) expect(r, LOCK_PENDING, v, "release with a successor not yet linked");
            else {
                expect(r, LOCK_CORRUPT, v, "release on a garbage last");
                if (a.mem != before) FAIL("release on last = %d wrote a word", v);
            }
            a.guards_intact("release on a garbage last");
        }
        // a garbage NEXT met by release and by the hand-off
        for (int signal = 0; signal < 2; ++signal) {
            Arena a(P);
            *a.last() = 3u;  // PE 2 is the tail, PE 1 releases
            const uint32_t next = (uint32_t)v & kNextMask;
            *a.data(1) = next | (signal ? kSignal : 0u);
            const std::vector<uint64_t> before = a.mem;
            const bool next_ok = next >= 1 && next <= (uint32_t)P;
            for (int which = 0; which < 2; ++which) {
                Arena b = a;
                for (int q = 0; q < P; ++q) b.table[(size_t)q] = (uint64_t)(uintptr_t)&b.mem[(size_t)(kGuard + q)];
                const Result r = which ? do_handoff(b, 1) : do_release(b, 1);
                const int prev = which ? 0 : 3;
                if (next == 0) {
                    expect(r, LOCK_PENDING, prev, "NEXT = 0");
                    if (b.mem != before) FAIL("PENDING changed a word");
                } else if (next_ok) {
                    expect(r, LOCK_HANDED, prev, "a valid NEXT");
                    if (!(*b.data((int)next - 1) & kSignal) && (int)next - 1 != 1) FAIL("no SIGNAL at PE %u", next - 1);
                } else {
                    expect(r, LOCK_CORRUPT, prev, "a garbage NEXT");
                    if (r.bad != (int32_t)next) FAIL("bad = %d, expected %u", r.bad, next);
                    if (b.mem != before) FAIL("a garbage NEXT = %u led to a store", next);
                }
                b.guards_intact("a garbage NEXT");
            }
        }
    }
}

int run_scripts()
{
    script_uncontended();
    script_queue_0_2_1();
    script_try_on_held();
    script_pending();
    script_corrupt();
    printf("lock_proto scripts: %d checks OK\n", g_checks);
    return 0;
}

// ---- threads ---------------------------------------------------------------------------

long g_counter = 0;  // NOT atomic: the lock is what orders the increments

void set_lock(Arena &a, int me)
{
    const Result r = do_enqueue(a, me);
    if (r.status == LOCK_CORRUPT) FAIL("PE %d: enqueue reports a corrupt lock (%d)", me, r.bad);
    if (r.status == LOCK_QUEUED)
        while (!(A::load(a.data(me)) & kSignal)) sched_yield();
}

void clear_lock(Arena &a, int me)
{
    Result r = do_release(a, me);
    if (r.status == LOCK_PENDING) {
        while (!(A::load(a.data(me)) & kNextMask)) sched_yield();
        r = do_handoff(a, me);
        if (r.status != LOCK_HANDED) FAIL("PE %d: hand-off after NEXT gives status %d", me, r.status);
    }
    if (r.status == LOCK_CORRUPT) FAIL("PE %d: release reports a corrupt lock (%d)", me, r.bad);
}

int run_threads(int P, int rounds)
{
    Arena a(P);
    g_counter = 0;
    std::vector<long> tries((size_t)P, 0);
    std::vector<std::thread> th;
    for (int me = 0; me < P; ++me)
        th.emplace_back([&a, me, rounds, &tries] {
            for (int k = 0; k < rounds; ++k) {
                if (k % 8 == 7) {
                    // every eighth round through try, bounded; a miss falls back to set
                    int n = 0;
                    bool got = false;
                    while (n++ < 64 && !(got = do_try(a, me).status == LOCK_ACQUIRED)) sched_yield();
                    tries[(size_t)me] += got;
                    if (!got) set_lock(a, me);
                } else {
                    set_lock(a, me);
                }
                ++g_counter;
                clear_lock(a, me);
            }
        });
    for (auto &t : th) t.join();
    if (g_counter != (long)P * rounds) FAIL("counter = %ld, expected %ld", g_counter, (long)P * rounds);
    for (int q = 0; q < P; ++q)
        if (a.mem[(size_t)(kGuard + q)] != 0) FAIL("PE %d's lock word is 0x%016llx at the end", q, (unsigned long long)a.mem[(size_t)(kGuard + q)]);
    a.guards_intact("threads");
    long t = 0;
    for (long v : tries) t += v;
    printf("lock_proto threads: P=%d rounds=%d counter=%ld (%ld through try) OK\n", P, rounds, g_counter, t);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "scripts")) return run_scripts();
    if (argc >= 4 && !strcmp(argv[1], "threads")) return run_threads(atoi(argv[2]), atoi(argv[3]));
    fprintf(stderr, "usage: %s scripts | threads P ROUNDS\n", argv[0]);
    return 2;
}
