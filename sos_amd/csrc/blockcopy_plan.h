// blockcopy_plan.h -- the host-side index split of sosx_block_strided_copy (blockcopy.hip)
// and the index decode its kernel shares with the CPU interpreter of
// tests/blockcopy_plan.cpp.  No HIP header: it compiles with a plain C++ compiler.
//
// Block i of the copy is bsize elements (bbytes = bsize * elem_size bytes) from
// src + i * sstride_b to dst + i * dstride_b.  A plan cuts every block the same way:
//
//   [0, head)                    element by element   (edge units)
//   [head, head + upb * width)   upb accesses of `width` bytes (body units)
//   [head + upb * width, bbytes) element by element   (edge units)
//
// and numbers the work flat: body unit w is access w % upb of block w / upb, so
// consecutive lanes run along a block and on into the next one (a block shorter than a
// wave's 64 accesses never leaves the rest of the wave idle); edge unit e is edge element
// e % epb of block e / epb.  A workgroup takes one tile of kBcTile units; the body tiles
// come first in the grid, the edge tiles after them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SOS_BC_HD __host__ __device__
#else
#define SOS_BC_HD
#endif

namespace sos {

enum BcRegime : int {
    BC_EMPTY = 0,        // nothing to move
    BC_CONTIGUOUS = 1,   // one run of bytes: sosx_strided_copy's contiguous form
    BC_ELEMENT = 2,      // single elements, one side contiguous: sosx_strided_copy pack/unpack
    BC_SMALL = 3,        // blocks under 16 B: one lane per element, lanes across blocks
    BC_CONGRUENT = 4,    // every block has one head / 16-B body / tail split on both sides
    BC_INCONGRUENT = 5,  // blocks of >= 16 B at differing offsets mod 16
};

constexpr unsigned kBcThreads = 256;  // == kThreads (elementwise.h)
constexpr unsigned kBcU = 4;          // accesses per lane and tile, all loaded before the first store
constexpr unsigned kBcTile = kBcThreads * kBcU;

struct BcPlan {
    int regime;
    int unaligned_loads;  // BC_INCONGRUENT: 16-B loads from 4-B-aligned addresses, aligned stores
    unsigned width;       // bytes per body access: 1, 2, 4, 8 or 16
    unsigned es;          // bytes per edge element (the element size after coarsening)
    uint64_t bbytes, nblocks;
    uint64_t sstride_b, dstride_b;  // byte strides
    uint64_t head, upb, tail;       // the split of one block (bytes, accesses, bytes)
    uint64_t he, epb;               // head elements and edge elements per block
    uint64_t body_units, edge_units;
    uint64_t body_wgs, edge_wgs;    // grid = body_wgs + edge_wgs
    // BC_CONTIGUOUS / BC_ELEMENT: the sosx_strided_copy call that moves the same bytes
    uint64_t d_count, d_es;
    int64_t d_dstr, d_sstr;
};

struct BcItem {
    uint64_t blk, j;
};

// Unit (w0 + off) of a flat numbering with `per` units per block, w0 the tile's first
// unit (uniform in a workgroup) and off < kBcTile.  The divisions of the lane part are
// 32-bit whenever per + kBcTile fits.
SOS_BC_HD inline BcItem bc_split(uint64_t w0, uint32_t off, uint64_t per)
{
    const uint64_t blk0 = w0 / per;
    const uint64_t r = w0 % per + off;
    if (r < per) return {blk0, r};
    if (per <= 0xffffffffull - kBcTile) {
        const uint32_t q = (uint32_t)r / (uint32_t)per;
        return {blk0 + q, (uint64_t)((uint32_t)r - q * (uint32_t)per)};
    }
    return {blk0 + r / per, r % per};
}

// Byte offset inside its block of body access j / of edge element k.
SOS_BC_HD inline uint64_t bc_body_offset(const BcPlan &p, uint64_t j) { return p.head + j * p.width; }
SOS_BC_HD inline uint64_t bc_edge_offset(const BcPlan &p, uint64_t k)
{
    return k < p.he ? k * p.es : p.head + p.upb * p.width + (k - p.he) * p.es;
}

inline uint64_t bc_lowbit(uint64_t v) { return v & (~v + 1); }

// The plan of one call; 0, or -3 (SOSX_ERR_ARG) for arguments the copy refuses.  Strides
// are in elements and >= bsize; both addresses are element-aligned.
inline int bc_plan(BcPlan *out, uintptr_t dst, ptrdiff_t dst_stride, uintptr_t src, ptrdiff_t src_stride,
                   size_t bsize, size_t nblocks, size_t elem_size)
{
    BcPlan p = {};
    *out = p;
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8 && elem_size != 16) return -3;
    if (dst_stride < 0 || src_stride < 0) return -3;
    if ((uint64_t)dst_stride < bsize || (uint64_t)src_stride < bsize) return -3;
    if (bsize == 0 || nblocks == 0) return 0;  // BC_EMPTY
    if (!dst || !src) return -3;
    if (dst % elem_size || src % elem_size) return -3;
    // the last block's byte offset and its end must fit 64 bits on either side
    const uint64_t big = (uint64_t)(dst_stride > src_stride ? dst_stride : src_stride);
    if ((uint64_t)nblocks > (UINT64_MAX / 32) / big) return -3;
    uint64_t es = elem_size, bs = bsize, dstr = (uint64_t)dst_stride, sstr = (uint64_t)src_stride;
    if (nblocks == 1) dstr = sstr = bs;  // one block: the strides move nothing
    p.nblocks = nblocks;
    p.bbytes = bs * es;
    p.sstride_b = sstr * es;
    p.dstride_b = dstr * es;
    if (dstr == bs && sstr == bs) {
        p.regime = BC_CONTIGUOUS;
        p.d_count = nblocks * bs;
        p.d_es = es;
        p.d_dstr = p.d_sstr = 1;
        *out = p;
        return 0;
    }
    const uint64_t all = (uint64_t)dst | (uint64_t)src | p.sstride_b | p.dstride_b;
    if (p.bbytes < 16) {
        // a block that is a power of two long and sits on its own grid on both sides is
        // one element of that size
        if ((p.bbytes & (p.bbytes - 1)) == 0 && all % p.bbytes == 0) {
            es = p.bbytes;
            bs = 1;
            dstr = p.dstride_b / es;
            sstr = p.sstride_b / es;
        }
        if (bs == 1 && (dstr == 1 || sstr == 1)) {
            p.regime = BC_ELEMENT;
            p.d_count = nblocks;
            p.d_es = es;
            p.d_dstr = (int64_t)dstr;
            p.d_sstr = (int64_t)sstr;
            *out = p;
            return 0;
        }
        p.regime = BC_SMALL;
        p.width = p.es = (unsigned)es;
        p.upb = bs;
    } else if (all % 16 == 0 || (p.sstride_b % 16 == 0 && p.dstride_b % 16 == 0 && (dst - src) % 16 == 0)) {
        p.regime = BC_CONGRUENT;
        p.width = 16;
        p.es = (unsigned)es;
        p.head = (16 - dst % 16) % 16;
        p.upb = (p.bbytes - p.head) / 16;
        p.tail = p.bbytes - p.head - p.upb * 16;
    } else {
        p.regime = BC_INCONGRUENT;
        p.es = (unsigned)es;
        const uint64_t w = bc_lowbit(all);  // < 16 here, >= es
        if (p.dstride_b % 16 == 0 && w >= 4) {
            // every target block has one split on the 16-B grid; the source vectors start
            // at multiples of 4 B
            p.unaligned_loads = 1;
            p.width = 16;
            p.head = (16 - dst % 16) % 16;
            p.upb = (p.bbytes - p.head) / 16;
            p.tail = p.bbytes - p.head - p.upb * 16;
        } else {
            p.width = (unsigned)w;
            p.upb = p.bbytes / w;
            p.tail = p.bbytes % w;
        }
    }
    p.he = p.head / p.es;
    p.epb = p.he + p.tail / p.es;
    p.body_units = nblocks * p.upb;
    p.edge_units = nblocks * p.epb;
    p.body_wgs = (p.body_units + kBcTile - 1) / kBcTile;
    p.edge_wgs = (p.edge_units + kBcTile - 1) / kBcTile;
    if (p.body_wgs + p.edge_wgs >= ((uint64_t)1 << 31)) return -3;
    *out = p;
    return 0;
}

}  // namespace sos
