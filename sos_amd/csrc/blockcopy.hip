// blockcopy.hip -- block-strided copy: block i of bsize elements goes from
// src + i * src_stride to dst + i * dst_stride (strides in elements, >= bsize), i < nblocks.
//
// The data movement of shmemx_ibput / shmemx_ibget (SOS issues one put or get per block,
// src/data_c.c4:499-524), with shmem_iput / shmem_iget as its bsize = 1 case; either
// side may be a peer's HBM mapped through the device heap.
//
// Three regimes, chosen on the host (blockcopy_plan.h bc_plan, which also holds the index
// decode that this kernel shares with the CPU interpreter of tests/blockcopy_plan.cpp):
//
//  * congruent -- blocks of >= 16 B, both byte strides multiples of 16 and src = dst
//    (mod 16): every block has the same head / 16-B body / tail split on both sides.  The
//    body moves as 16-B nontemporal loads and stores, lanes along the block; the body
//    vectors of all blocks are numbered flat, so a wave runs on into the next block when
//    a block is shorter than its 1 KiB.
//  * incongruent -- blocks of >= 16 B whose source and target, or successive blocks, sit
//    at different offsets mod 16.  The accesses are the widest power of two that divides
//    both base addresses and both byte strides.  Where the target's stride is a multiple
//    of 16 B and that width is at least 4 B, the target side keeps the 16-B path: aligned
//    nontemporal 16-B stores on the target's grid, each fed by ONE unaligned 16-B load
//    (ldv_unaligned, the UL form of DESIGN.md section 4.1).  UL and not the DPP next-lane
//    form: a lane's source vector may continue in the next BLOCK, which is not the next
//    lane's load, so the DPP form would need a second load at every block end; and the
//    gather measured UL ahead of DPP for sources at 4-B multiples
//    (profiles/r6_gather_realign_ab.txt).  Below 4 B, where the unaligned load is untested
//    (DESIGN.md section 9 item 3), and for a target stride off the 16-B grid the copy
//    uses the common width on both sides.
//  * small -- blocks under 16 B (shmem_iput / iget): one lane per element, lanes across
//    blocks, plain (cached) accesses as in strided.hip's both-strided form: neighbouring
//    lanes share the lines they touch.  A block that is a power of two long and on its own
//    grid is treated as one element of that size; single elements with one side contiguous
//    are sosx_strided_copy's pack / unpack, and a copy whose blocks abut on both sides is
//    its contiguous form.
//
// Launch shape as strided.hip and combine.hip: one tile per workgroup (kBcU accesses per
// lane), every load of the tile issued before its first store, no grid-stride loop.  The
// ragged head and tail of the blocks go element by element in workgroups of their own
// at the end of the grid.  No access overhangs a block: bytes between target blocks are
// never written, and none is read and written back.
#include "blockcopy_plan.h"
#include "elementwise.h"

namespace sos {

static_assert(kBcThreads == (unsigned)kThreads, "blockcopy_plan.h mirrors kThreads");

template <class A, bool NT, bool UL> __device__ __forceinline__ A bc_load(const char *p)
{
    if constexpr (UL) return ldv_unaligned(p);
    else if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const A *>(p));
    else return *reinterpret_cast<const A *>(p);
}

template <class A, bool NT> __device__ __forceinline__ void bc_store(char *p, A v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<A *>(p));
    else *reinterpret_cast<A *>(p) = v;
}

// A: the body's access type; E: the element type of the edges
template <class A, class E, bool NT, bool UL>
__global__ __launch_bounds__(kThreads) void k_block_copy(char *dst, const char *src, BcPlan p)
{
    if (blockIdx.x < p.body_wgs) {
        const uint64_t w0 = (uint64_t)blockIdx.x * kBcTile;
        A v[kBcU];
        uint64_t doff[kBcU];
#pragma unroll
        for (unsigned u = 0; u < kBcU; ++u) {
            const uint32_t off = threadIdx.x + u * kBcThreads;
            if (w0 + off < p.body_units) {
                const BcItem it = bc_split(w0, off, p.upb);
                const uint64_t in = bc_body_offset(p, it.j);
                doff[u] = it.blk * p.dstride_b + in;
                v[u] = bc_load<A, NT, UL>(src + it.blk * p.sstride_b + in);
            }
        }
#pragma unroll
        for (unsigned u = 0; u < kBcU; ++u)
            if (w0 + threadIdx.x + u * kBcThreads < p.body_units) bc_store<A, NT>(dst + doff[u], v[u]);
    } else {
        const uint64_t e0 = ((uint64_t)blockIdx.x - p.body_wgs) * kBcTile;
        E v[kBcU];
        uint64_t doff[kBcU];
#pragma unroll
        for (unsigned u = 0; u < kBcU; ++u) {
            const uint32_t off = threadIdx.x + u * kBcThreads;
            if (e0 + off < p.edge_units) {
                const BcItem it = bc_split(e0, off, p.epb);
                const uint64_t in = bc_edge_offset(p, it.j);
                doff[u] = it.blk * p.dstride_b + in;
                v[u] = *reinterpret_cast<const E *>(src + it.blk * p.sstride_b + in);
            }
        }
#pragma unroll
        for (unsigned u = 0; u < kBcU; ++u)
            if (e0 + threadIdx.x + u * kBcThreads < p.edge_units) *reinterpret_cast<E *>(dst + doff[u]) = v[u];
    }
}

}  // namespace sos

using namespace sos;

namespace {

template <class A, class E, bool NT, bool UL> int launch(char *dst, const char *src, const BcPlan &p, hipStream_t st)
{
    hipLaunchKernelGGL((k_block_copy<A, E, NT, UL>), dim3((unsigned)(p.body_wgs + p.edge_wgs)), dim3(kThreads),
                       0, st, dst, src, p);
    return hip_ok(hipGetLastError());
}

// the body's access width (<= 16 B, >= the element size); a plan that names a width below
// its element size has no kernel and is refused, not skipped
template <class E, bool NT> int launch_width(char *dst, const char *src, const BcPlan &p, hipStream_t st)
{
    if (p.unaligned_loads) return launch<u32x4, E, true, true>(dst, src, p, st);
    switch (p.width) {
        case 16: return launch<u32x4, E, NT, false>(dst, src, p, st);
        case 8: if constexpr (sizeof(E) <= 8) return launch<uint64_t, E, NT, false>(dst, src, p, st); break;
        case 4: if constexpr (sizeof(E) <= 4) return launch<uint32_t, E, NT, false>(dst, src, p, st); break;
        case 2: if constexpr (sizeof(E) <= 2) return launch<uint16_t, E, NT, false>(dst, src, p, st); break;
        case 1: if constexpr (sizeof(E) <= 1) return launch<uint8_t, E, NT, false>(dst, src, p, st); break;
        default: break;
    }
    return SOSX_ERR_ARG;
}

template <bool NT> int launch_elem(char *dst, const char *src, const BcPlan &p, hipStream_t st)
{
    switch (p.es) {
        case 1: return launch_width<uint8_t, NT>(dst, src, p, st);
        case 2: return launch_width<uint16_t, NT>(dst, src, p, st);
        case 4: return launch_width<uint32_t, NT>(dst, src, p, st);
        case 8: return launch_width<uint64_t, NT>(dst, src, p, st);
        case 16: return launch_width<u32x4, NT>(dst, src, p, st);
        default: return SOSX_ERR_ARG;
    }
}

}  // namespace

extern "C" int sosx_block_strided_copy(void *dst, ptrdiff_t dst_stride, const void *src, ptrdiff_t src_stride,
                                       size_t bsize, size_t nblocks, size_t elem_size, void *stream)
{
    // every argument is checked before any device work
    BcPlan p;
    const int rc = bc_plan(&p, (uintptr_t)dst, dst_stride, (uintptr_t)src, src_stride, bsize, nblocks, elem_size);
    if (rc != 0) return SOSX_ERR_ARG;
    switch (p.regime) {
        case BC_EMPTY: return SOSX_OK;
        case BC_CONTIGUOUS:
        case BC_ELEMENT:
            return sosx_strided_copy(dst, (ptrdiff_t)p.d_dstr, src, (ptrdiff_t)p.d_sstr, (size_t)p.d_es,
                                     (size_t)p.d_count, stream);
        case BC_SMALL: return launch_elem<false>((char *)dst, (const char *)src, p, as_stream(stream));
        default: return launch_elem<true>((char *)dst, (const char *)src, p, as_stream(stream));
    }
}

// The plan of a call as the library would run it (tests, tools): regime, access width,
// unaligned loads, head / body accesses / tail of a block, workgroups.
extern "C" int sosx_block_copy_plan(uintptr_t dst, ptrdiff_t dst_stride, uintptr_t src, ptrdiff_t src_stride,
                                    size_t bsize, size_t nblocks, size_t elem_size, long long out[8])
{
    BcPlan p;
    const int rc = bc_plan(&p, dst, dst_stride, src, src_stride, bsize, nblocks, elem_size);
    if (rc != 0 || !out) return SOSX_ERR_ARG;
    out[0] = p.regime;
    out[1] = p.width;
    out[2] = p.unaligned_loads;
    out[3] = (long long)p.head;
    out[4] = (long long)p.upb;
    out[5] = (long long)p.tail;
    out[6] = (long long)p.body_wgs;
    out[7] = (long long)p.edge_wgs;
    return SOSX_OK;
}
