// p2p_proto_collect_harness.cpp -- collect plans (PLAN_COLLECT: per-PE byte lengths)
// through the p2p transport's pairing protocol on CPU threads, for ThreadSanitizer.
//
// Test infrastructure (tests/test_p2p_proto_collect.py builds and runs it; no GPU).  The
// backend -- per-PE "stream" worker, heaps, the consumer-side acquire check -- is the one of
// tests/p2p_proto_harness.cpp, compiled into this translation unit with its main()
// renamed; this file adds the collect calls, whose plans and whose peers' plans
// (sosp2p::peer_sends) are built from the lengths every PE holds.  Every result is checked
// against the concatenation, and the word above it must keep its sentinel.
//
// Usage: p2p_proto_collect_harness [iters]   prints "... N collect calls OK", exit 0
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#define main p2p_proto_harness_main
#include "p2p_proto_harness.cpp"
#undef main

namespace {

// Per-PE lengths in 4-byte words, by pattern: 0 = all equal, 1 = alternating zero and
// odd lengths, 2 = one long among short (some zero), 3 = only the last PE contributes,
// 4 = all zero (no rounds: the protocol is not entered).
uint64_t collect_words(int pattern, int q, int P)
{
    static const uint64_t odd[] = {1, 3, 15, 17, 255};
    switch (pattern) {
        case 0: return 5;
        case 1: return q % 2 ? odd[(q / 2) % 5] : 0;
        case 2: return q == P / 2 ? 65539 : (uint64_t)(q % 3);
        case 3: return q == P - 1 ? 1001 : 0;
        default: return 0;
    }
}

struct CollectCase {
    int pattern;
    unsigned soff, doff;  // byte offsets of src/dst in their heap regions
};

void collect_pe_main(int P, int me, int mode, const std::vector<CollectCase> &cases,
                     sosp2p::Shared *sh, long *ok_calls)
{
    Stream st;
    const bool stream_mode = mode > 0;
    CpuBackend be{&st, mode == 1 || (mode == 3 && me % 2 == 0), me, sh, {}};
    sosp2p::Local loc;
    sosp2p::StreamLocal sl;
    char *heap = g_heaps[(size_t)me];
    const size_t region = kHeap / 4;
    const int alg = SOSX_PLAN_COLLECT;
    uint64_t call = 0;
    for (const CollectCase &c : cases) {
        ++call;
        uint64_t lens[sosp2p::kMaxPE], words = 0;
        for (int q = 0; q < P; ++q) {
            lens[q] = 4 * collect_words(c.pattern, q, P);
            words += lens[q] / 4;
        }
        if (4 * (words + 1) + c.doff > region) die("heap too small", (int)words);
        char *src = heap + c.soff, *dst = heap + region + c.doff;
        // this call's source and sentinels (the caller's writes, after the previous call returned)
        for (uint64_t i = 0; i < lens[me] / 4; ++i) {
            const uint32_t v = val(call, me, i);
            memcpy(src + 4 * i, &v, 4);
        }
        const uint32_t sentinel = 0xA5A5A5A5u;
        for (uint64_t i = 0; i <= words; ++i) memcpy(dst + 4 * i, &sentinel, 4);
        const unsigned smis = (unsigned)((uintptr_t)src & 15), dmis = (unsigned)((uintptr_t)dst & 15);
        sosplan::Plan plan;
        if (sosplan::build(alg, P, me, 0, 1, smis, dmis, &plan, lens) != SOSX_OK) die("plan", alg, P);
        if (plan.scratch_bytes || plan.src_bytes != lens[me] || plan.dst_bytes != 4 * words)
            die("collect extents");
        const sosp2p::Bufs b{src, dst, nullptr, (uint64_t)(src - heap), (uint64_t)(dst - heap), 0, smis, dmis};
        auto world_of = [](int i) { return i; };
        const int rc = stream_mode
                           ? sosp2p::exec_stream(plan, P, me, world_of, alg, 0, 1, b, sh, sl, be, lens)
                           : sosp2p::exec_host(plan, P, me, world_of, alg, 0, 1, b, sh, loc, be, lens);
        if (rc) die("exec failed", rc);
        uint64_t at = 0;
        uint32_t got;
        for (int q = 0; q < P; ++q)
            for (uint64_t i = 0; i < lens[q] / 4; ++i, ++at) {
                memcpy(&got, dst + 4 * at, 4);
                if (got != val(call, q, i)) die("wrong result", c.pattern, (int)at);
            }
        memcpy(&got, dst + 4 * words, 4);
        if (got != sentinel) die("collect wrote above the sum of the lengths", c.pattern);
        ++*ok_calls;
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 2;
    long total = 0;
    auto *sh = (sosp2p::Shared *)calloc(1, sizeof(sosp2p::Shared));
    for (int mode = 0; mode < 4; ++mode)
        for (int P : {2, 3, 4, 5, 8, 12}) {
            g_heaps.clear();
            for (int q = 0; q < P; ++q) {
                char *h = (char *)aligned_alloc(4096, kHeap);
                memset(h, 0, kHeap);
                g_heaps.push_back(h);
            }
            std::vector<CollectCase> cases;
            for (int it = 0; it < 4 * iters; ++it)
                for (int pattern = 0; pattern < 5; ++pattern)
                    cases.push_back(CollectCase{pattern, 4u * (unsigned)it % 16, pattern == 1 ? 4u : 0u});
            memset((void *)sh, 0, sizeof(*sh));  // fresh counters: a new job
            std::vector<long> ok((size_t)P, 0);
            std::vector<std::thread> th;
            for (int q = 0; q < P; ++q)
                th.emplace_back(collect_pe_main, P, q, mode, std::cref(cases), sh, &ok[(size_t)q]);
            for (auto &t : th) t.join();
            for (long v : ok) total += v;
            for (char *h : g_heaps) free(h);
        }
    free(sh);
    if (g_peer_reads.load() == 0) die("no launch read a peer's bytes");
    printf("p2p protocol collect harness: %ld collect calls OK (host and stream signalling, both "
           "entries); %ld peer reads, each after an acquire (%ld acquires)\n", total,
           g_peer_reads.load(), g_acquires.load());
    return 0;
}
