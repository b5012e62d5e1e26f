// strided.hip -- strided element copy: dst[k * dst_stride] = src[k * src_stride], k < count.
//
// The pack and unpack passes of shmem_alltoalls (src/collectives.c:1483-1531): SOS moves
// element k of a block from `sst` elements apart in the source to `dst` elements apart in
// the target.  Here the whole operand is packed once (P * nelems elements at stride sst),
// exchanged as a contiguous alltoall, and unpacked once at stride dst.
//
// Lane mapping: on the contiguous side a lane owns ONE 16-B vector (V = 16 / elem_size
// elements), consecutive lanes consecutive vectors, so that side moves as full 1 KiB
// nontemporal wave accesses on its own 16-B grid.  The lane's V element accesses on the
// strided side are `stride` elements apart and the wave's 64 * V elements cover one
// contiguous span of 64 * V * stride elements: every cache line the wave touches there is
// used up by the wave's own V back-to-back instructions (a line is fetched once and the
// later instructions hit it in the CU's cache), where "lane k takes element k" would
// need a cross-lane transpose to form the 16-B vectors.  Strided accesses are plain
// (cached) for that reason; only the contiguous side is nontemporal.
//
// Launch shape as the combine's: one tile per workgroup, every load of the tile issued
// before its first store, no grid-stride loop.  The ragged head and tail around the
// 16-B body go element by element in the last workgroup.  The unpack and both-strided
// forms store single elements only: bytes between target elements are never written.
#include "elementwise.h"

namespace sos {

// 16-B vectors per lane per tile: at most 16 element loads in flight per lane
template <class T> constexpr int strided_u()
{
    return sizeof(T) == 1 ? 1 : sizeof(T) == 2 ? 2 : 4;
}

// dst contiguous (16-B nontemporal stores on dst's grid), src strided
template <class T, int U>
__global__ __launch_bounds__(kThreads) void k_strided_pack(T *dst, const T *src, uint64_t sst,
                                                           uint64_t head, uint64_t nvec,
                                                           uint64_t count)
{
    constexpr int V = 16 / (int)sizeof(T);
    u32x4 *body = reinterpret_cast<u32x4 *>(dst + head);
    const T *sb = src + head * sst;
    const uint64_t j0 = (uint64_t)blockIdx.x * (uint64_t)(kThreads * U) + threadIdx.x;
    T e[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t j = j0 + (uint64_t)u * kThreads;
        if (j < nvec) {
#pragma unroll
            for (int i = 0; i < V; ++i) e[u][i] = sb[(j * V + (uint64_t)i) * sst];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t j = j0 + (uint64_t)u * kThreads;
        if (j < nvec) {
            u32x4 v;
            __builtin_memcpy(&v, e[u], 16);
            __builtin_nontemporal_store(v, body + j);
        }
    }
    if (blockIdx.x == gridDim.x - 1) {
        for (uint64_t k = threadIdx.x; k < head; k += kThreads) dst[k] = src[k * sst];
        for (uint64_t k = head + nvec * V + threadIdx.x; k < count; k += kThreads) dst[k] = src[k * sst];
    }
}

// src contiguous (16-B nontemporal loads on src's grid), dst strided: element stores only
template <class T, int U>
__global__ __launch_bounds__(kThreads) void k_strided_unpack(T *dst, uint64_t dstr, const T *src,
                                                             uint64_t head, uint64_t nvec,
                                                             uint64_t count)
{
    constexpr int V = 16 / (int)sizeof(T);
    const u32x4 *body = reinterpret_cast<const u32x4 *>(src + head);
    T *db = dst + head * dstr;
    const uint64_t j0 = (uint64_t)blockIdx.x * (uint64_t)(kThreads * U) + threadIdx.x;
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t j = j0 + (uint64_t)u * kThreads;
        if (j < nvec) v[u] = __builtin_nontemporal_load(body + j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t j = j0 + (uint64_t)u * kThreads;
        if (j < nvec) {
            T e[V];
            __builtin_memcpy(e, &v[u], 16);
#pragma unroll
            for (int i = 0; i < V; ++i) db[(j * V + (uint64_t)i) * dstr] = e[i];
        }
    }
    if (blockIdx.x == gridDim.x - 1) {
        for (uint64_t k = threadIdx.x; k < head; k += kThreads) dst[k * dstr] = src[k];
        for (uint64_t k = head + nvec * V + threadIdx.x; k < count; k += kThreads) dst[k * dstr] = src[k];
    }
}

// both strided: lane k of the tile takes element k
constexpr int kStridedElemU = 4;

template <class T>
__global__ __launch_bounds__(kThreads) void k_strided_elem(T *dst, uint64_t dstr, const T *src,
                                                           uint64_t sst, uint64_t count)
{
    const uint64_t k0 = (uint64_t)blockIdx.x * (uint64_t)(kThreads * kStridedElemU) + threadIdx.x;
    T e[kStridedElemU];
#pragma unroll
    for (int u = 0; u < kStridedElemU; ++u) {
        const uint64_t k = k0 + (uint64_t)u * kThreads;
        if (k < count) e[u] = src[k * sst];
    }
#pragma unroll
    for (int u = 0; u < kStridedElemU; ++u) {
        const uint64_t k = k0 + (uint64_t)u * kThreads;
        if (k < count) dst[k * dstr] = e[u];
    }
}

}  // namespace sos

using namespace sos;

namespace {

// elements before the first 16-B boundary of a contiguous operand (a multiple of the
// element size away: the pointer is element-aligned), capped at count
template <class T> uint64_t head_elems(const void *p, uint64_t count)
{
    const uint64_t h = ((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T);
    return h < count ? h : count;
}

template <class T>
int launch_strided(void *dst, uint64_t dstr, const void *src, uint64_t sst, uint64_t count,
                   hipStream_t st)
{
    constexpr int U = strided_u<T>();
    constexpr uint64_t V = 16 / sizeof(T);
    T *d = (T *)dst;
    const T *s = (const T *)src;
    if (dstr == 1 || sst == 1) {
        const bool pack = dstr == 1;
        const uint64_t head = head_elems<T>(pack ? dst : src, count);
        const uint64_t nvec = (count - head) / V;
        const uint64_t tile = (uint64_t)kThreads * U;
        uint64_t blocks = (nvec + tile - 1) / tile;
        if (!blocks) blocks = 1;  // the ragged ends alone
        if (blocks > 0xffffffffull) return SOSX_ERR_ARG;
        if (pack)
            hipLaunchKernelGGL((k_strided_pack<T, U>), dim3((unsigned)blocks), dim3(kThreads), 0, st, d,
                               s, sst, head, nvec, count);
        else
            hipLaunchKernelGGL((k_strided_unpack<T, U>), dim3((unsigned)blocks), dim3(kThreads), 0, st, d,
                               dstr, s, head, nvec, count);
    } else {
        const uint64_t tile = (uint64_t)kThreads * kStridedElemU;
        const uint64_t blocks = (count + tile - 1) / tile;
        if (blocks > 0xffffffffull) return SOSX_ERR_ARG;
        hipLaunchKernelGGL((k_strided_elem<T>), dim3((unsigned)blocks), dim3(kThreads), 0, st, d, dstr, s,
                           sst, count);
    }
    return hip_ok(hipGetLastError());
}

}  // namespace

extern "C" int sosx_strided_copy(void *dst, ptrdiff_t dst_stride, const void *src,
                                 ptrdiff_t src_stride, size_t elem_size, size_t count, void *stream)
{
    // every argument is checked before any device work
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8 && elem_size != 16)
        return SOSX_ERR_ARG;
    if (dst_stride < 1 || src_stride < 1) return SOSX_ERR_ARG;
    if (count == 0) return SOSX_OK;
    if (!dst || !src) return SOSX_ERR_ARG;
    if ((uintptr_t)dst % elem_size || (uintptr_t)src % elem_size) return SOSX_ERR_ARG;
    // the last element's byte offset must fit 64 bits on either side
    const uint64_t dstr = (uint64_t)dst_stride, sst = (uint64_t)src_stride;
    const uint64_t big = dstr > sst ? dstr : sst;
    if ((uint64_t)count > (UINT64_MAX / 16) / big) return SOSX_ERR_ARG;
    hipStream_t st = as_stream(stream);
    if (dstr == 1 && sst == 1) {  // contiguous: the gather's one-segment copy
        const void *srcs[1] = {src};
        void *dsts[1] = {dst};
        const size_t bytes[1] = {count * elem_size};
        return sosx_gather(1, srcs, dsts, bytes, stream);
    }
    switch (elem_size) {
        case 1: return launch_strided<uint8_t>(dst, dstr, src, sst, count, st);
        case 2: return launch_strided<uint16_t>(dst, dstr, src, sst, count, st);
        case 4: return launch_strided<uint32_t>(dst, dstr, src, sst, count, st);
        case 8: return launch_strided<uint64_t>(dst, dstr, src, sst, count, st);
        default: return launch_strided<u32x4>(dst, dstr, src, sst, count, st);
    }
}
