// putsignal_plan.h -- the host-side split of sosx_put_signal's copy (putsignal.hip).  No HIP
// header: it compiles with a plain C++ compiler (tests/sync_eval_harness.cpp sweeps it).
//
// The payload [0, nbytes) is cut as blockcopy_plan.h cuts one block:
//
//   [0, head)                       byte by byte          (edge)
//   [head, head + units * width)    units accesses of `width` bytes (body)
//   [head + units * width, nbytes)  byte by byte          (edge)
//
//  * congruent -- source = target (mod 16): head brings the target to its 16-B grid, the
//    body moves as aligned 16-B loads and stores;
//  * incongruent, both on a 4-B grid -- the target side keeps aligned 16-B stores, each fed
//    by one unaligned 16-B load (blockcopy.hip's UL form);
//  * incongruent below 4 B -- the widest power of two dividing both addresses, on both sides.
//
// A workgroup takes tiles of kPsTile body units, grid-stride; the grid is one workgroup per
// tile up to kPsMaxGrid (one per CU of an MI355X).  No access leaves [0, nbytes).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sos {

constexpr unsigned kPsThreads = 256;
constexpr unsigned kPsU = 2;  // accesses per lane and tile, all loaded before the first store
constexpr unsigned kPsTile = kPsThreads * kPsU;
constexpr unsigned kPsMaxGrid = 256;

struct PsPlan {
    unsigned width;  // bytes per body access: 1, 2, 4, 8 or 16
    int unaligned_loads;
    uint64_t head, units, tail;
    uint64_t tiles;
    unsigned grid;
};

inline PsPlan ps_plan(uintptr_t dst, uintptr_t src, size_t nbytes)
{
    PsPlan p = {};
    p.width = 16;
    p.grid = 1;
    if (!nbytes) return p;
    const uint64_t to_grid = (16 - dst % 16) % 16;
    if ((dst - src) % 16 == 0) {
        p.head = to_grid < nbytes ? to_grid : nbytes;
        p.units = (nbytes - p.head) / 16;
    } else {
        const uint64_t all = (uint64_t)dst | (uint64_t)src;
        const uint64_t w = all & (~all + 1);  // < 16 here
        if (w >= 4) {
            p.unaligned_loads = 1;
            p.head = to_grid < nbytes ? to_grid : nbytes;
            p.units = (nbytes - p.head) / 16;
        } else {
            p.width = (unsigned)w;
            p.units = nbytes / w;
        }
    }
    p.tail = nbytes - p.head - p.units * p.width;
    p.tiles = (p.units + kPsTile - 1) / kPsTile;
    p.grid = p.tiles > kPsMaxGrid ? kPsMaxGrid : (p.tiles ? (unsigned)p.tiles : 1u);
    return p;
}

}  // namespace sos
