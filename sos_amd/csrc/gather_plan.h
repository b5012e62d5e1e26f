// gather_plan.h -- the host-side split of sosx_gather / sosx_gather_signalled (copy.hip):
// the per-launch geometry k_gather reads, the grouping of segments into launches and the
// placement of the signalling step (the gate).  No HIP header: it compiles with a plain C++
// compiler (tests/gather_plan.cpp walks every launch as the workgroups do).
//
// A segment of `bytes` from src to dst is cut on the DESTINATION's 16-B grid:
//
//   [0, head)                     byte by byte             (the launch's last workgroup)
//   [head, head + nvec * 16)      nvec aligned 16-B stores (one tile of kTileVec per workgroup)
//   [head + nvec * 16, bytes)     byte by byte             (the launch's last workgroup)
//
// sd is the source's offset inside its own 16-B grid at the body's start: 0 -- aligned
// loads; a multiple of 4 with `ul` -- one unaligned 16-B load per vector; otherwise the
// aligned vectors j and j + 1, funnel-shifted (the DPP form).  Every aligned load holds at
// least one byte of its segment, so none touches a page the segment does not.
//
// Zero-byte segments take no slot.  The live segments go, in order, into launches of at
// most kMaxSeg slots, EACH SEGMENT INTO EXACTLY ONE LAUNCH: a launch starts at the segment
// after the last one the launch before it looked at.  A launch's grid is one workgroup per
// tile, at least one (the last workgroup also runs the byte loops).
//
// The gate rides in the copy launch (GG_FUSED) only when all live segments fit ONE launch
// of at most kGateMaxBlocks workgroups; otherwise it is its own launch before the first
// copy (GG_STEP_BEFORE), and when nothing is copied its own launch alone (GG_STEP_ALONE).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef GATHER_U
#define GATHER_U 4
#endif

namespace sos {

constexpr int kMaxSeg = 16;
constexpr unsigned kGateMaxBlocks = 16;
constexpr unsigned kGatherThreads = 256;  // == kThreads (elementwise.h)
// One tile of kGatherU 16-B vectors per lane, one tile per workgroup.
constexpr int kGatherU = GATHER_U;
constexpr uint64_t kTileVec = (uint64_t)kGatherThreads * kGatherU;

enum GatherGate : int {
    GG_NONE = 0,         // no gate, or this launch owes it nothing
    GG_FUSED = 1,        // the launch carries the signalling step (k_gather<true>)
    GG_STEP_BEFORE = 2,  // the step as its own launch, right before this copy launch
    GG_STEP_ALONE = 3,   // nothing copied: the step as the call's only launch
};

// One launch: what GatherArgs carries besides the addresses, and which of the caller's
// segments sits in each slot.
struct GatherLaunch {
    int seg[kMaxSeg];
    uint64_t head[kMaxSeg];    // bytes before the 16-B aligned body (of dst)
    unsigned sd[kMaxSeg];      // src's offset within its aligned vectors there (0: congruent)
    uint64_t nvec[kMaxSeg];    // 16-B vectors in the body
    uint64_t bytes[kMaxSeg];
    uint64_t tstart[kMaxSeg + 1];  // prefix sums of each segment's tiles
    int nseg;
    int ul;                    // incongruent sources at 4-B offsets: unaligned loads
    uint64_t blocks;           // the grid: max(1, tiles)
    int gate;                  // GG_NONE, GG_FUSED or GG_STEP_BEFORE
};

struct GatherCursor {
    int next;          // the first segment no launch has looked at yet
    int live;          // segments of at least one byte
    int gate_pending;  // a gate nobody has placed yet; after the last launch: GG_STEP_ALONE
};

inline GatherCursor gather_begin(int nseg, const size_t *bytes, bool gated)
{
    GatherCursor c = {0, 0, gated ? 1 : 0};
    for (int i = 0; i < nseg; ++i) c.live += bytes[i] != 0;
    return c;
}

// Packs the next launch: 1, 0 when no live segment is left, -3 (SOSX_ERR_ARG) for a grid
// past 32 bits.  AS and AD: pointer types or uintptr_t.
template <class AS, class AD>
inline int gather_next(GatherCursor *c, GatherLaunch *out, int nseg, const AS *srcs, const AD *dsts,
                       const size_t *bytes, bool ul)
{
    GatherLaunch g = {};
    int n = 0, i = c->next;
    uint64_t tot = 0;
    for (; i < nseg && n < kMaxSeg; ++i) {
        if (!bytes[i]) continue;
        const uintptr_t s = (uintptr_t)srcs[i], d = (uintptr_t)dsts[i];
        g.seg[n] = i;
        g.bytes[n] = bytes[i];
        // the body on dst's 16-B grid; an incongruent src is realigned in registers
        uint64_t h = (16 - (d & 15)) & 15;
        if (h > bytes[i]) h = bytes[i];
        g.head[n] = h;
        g.nvec[n] = (bytes[i] - h) / 16;
        g.sd[n] = (unsigned)((s + h) & 15);
        g.tstart[n] = tot;
        tot += (g.nvec[n] + kTileVec - 1) / kTileVec;
        ++n;
    }
    c->next = i;  // the launch after this one starts where this one stopped
    if (!n) return 0;
    g.nseg = n;
    g.tstart[n] = tot;
    g.ul = ul ? 1 : 0;
    g.blocks = tot ? tot : 1;  // one tile per workgroup (+ the ragged ends)
    if (g.blocks > 0xffffffffull) return -3;
    if (c->gate_pending) {
        g.gate = c->live <= kMaxSeg && g.blocks <= kGateMaxBlocks ? GG_FUSED : GG_STEP_BEFORE;
        c->gate_pending = 0;
    }
    *out = g;
    return 1;
}

// The whole call at a glance (sosx_gather_plan).
struct GatherSummary {
    long long launches, tiles, live, slots;
    int gate;  // where the gate goes; GG_NONE without one
    long long first_blocks, last_blocks;
};

template <class AS, class AD>
inline int gather_summary(GatherSummary *out, int nseg, const AS *srcs, const AD *dsts, const size_t *bytes,
                          bool gated, bool ul)
{
    GatherSummary s = {};
    GatherCursor c = gather_begin(nseg, bytes, gated);
    GatherLaunch g;
    int rc;
    while ((rc = gather_next(&c, &g, nseg, srcs, dsts, bytes, ul)) == 1) {
        if (!s.launches++) s.first_blocks = (long long)g.blocks;
        s.last_blocks = (long long)g.blocks;
        s.tiles += (long long)g.tstart[g.nseg];
        s.slots += g.nseg;
        if (g.gate != GG_NONE) s.gate = g.gate;
    }
    if (rc != 0) return rc;
    if (c.gate_pending) s.gate = GG_STEP_ALONE;
    s.live = c.live;
    *out = s;
    return 0;
}

}  // namespace sos
