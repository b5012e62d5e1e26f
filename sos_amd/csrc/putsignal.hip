// putsignal.hip -- the device side of put-with-signal and of the point-to-point waits
// (signal.cpp): sosx_put_signal and sosx_sync_snapshot.
//
// sosx_put_signal: ONE launch copies nbytes from source to target and then updates the
// 64-bit signal word, the update visible no earlier than the payload.  Either pointer may be
// this PE's HBM, a peer's HBM mapped through the device heap, or host memory HIP allocated
// or registered (its device view).
//
//  * copy: the split of putsignal_plan.h -- aligned 16-B accesses where source and target
//    are congruent mod 16, else aligned 16-B stores fed by unaligned 16-B loads (4-B grids)
//    or the common width; tiles grid-stride, every load of a tile before its first store; the
//    ragged head and tail byte by byte in workgroup 0.  No access overhangs the payload.
//  * hand-off, the producer form carried to system scope: every storing wave waits for its
//    stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, lane 0 issues a
//    system-scope release fence and the explicit s_waitcnt vmcnt(0) again (the compiler may
//    drop the fence's own wait when it can prove the wave's scoreboard empty; inline asm it
//    does not see), then adds 1 at agent scope to a ticket word in device memory.
//  * signal: the workgroup whose add returned gridDim.x - 1 is the last; its lane 0 performs
//    the update -- a system-scope exchange (SET) or fetch_add (ADD), as amo.hip does an
//    atomic -- and stores 0 to the ticket for the next launch.  Launches that share a ticket
//    must be serial: the library stream's share the library's word, and every created
//    context brings its own (sosx_put_signal_on).
//
// Nothing here waits on memory: no loop polls a word.
//
// sosx_sync_snapshot: nelems words of 2, 4 or 8 bytes from device memory into a pinned host
// buffer, one lane per word, grid-stride; each word is read ONCE with a relaxed
// system-scope atomic load and stored with a plain vector store.  No fence: the host reads
// the buffer after the stream's next system-scope release (sync_system).
#include "elementwise.h"
#include "putsignal_plan.h"

namespace sos {

static_assert(kPsThreads == (unsigned)kThreads, "putsignal_plan.h mirrors kThreads");

template <class A, bool UL>
__global__ __launch_bounds__(kThreads) void k_put_signal(char *dst, const char *src, PsPlan p, uint64_t *sig,
                                                         uint64_t value, int sig_op, unsigned *ticket)
{
    for (uint64_t t = blockIdx.x; t < p.tiles; t += gridDim.x) {
        const uint64_t u0 = t * kPsTile;
        A v[kPsU];
#pragma unroll
        for (unsigned u = 0; u < kPsU; ++u) {
            const uint64_t i = u0 + threadIdx.x + u * kPsThreads;
            if (i < p.units) {
                const char *s = src + p.head + i * sizeof(A);
                if constexpr (UL) v[u] = ldv_unaligned(s);
                else v[u] = *reinterpret_cast<const A *>(s);
            }
        }
#pragma unroll
        for (unsigned u = 0; u < kPsU; ++u) {
            const uint64_t i = u0 + threadIdx.x + u * kPsThreads;
            if (i < p.units) *reinterpret_cast<A *>(dst + p.head + i * sizeof(A)) = v[u];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < p.head + p.tail) {
        const uint64_t k = threadIdx.x;
        const uint64_t off = k < p.head ? k : p.head + p.units * sizeof(A) + (k - p.head);
        dst[off] = src[off];
    }
    // the hand-off: stores drained in every wave, then one release for the workgroup
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned arrived = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived != gridDim.x - 1) return;
    if (sig_op == SOSX_SIGNAL_SET)
        (void)__hip_atomic_exchange(sig, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else
        (void)__hip_atomic_fetch_add(sig, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class T> __device__ __forceinline__ T snapshot_load(const T *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <class T>
__global__ __launch_bounds__(kThreads) void k_sync_snapshot(T *out, const T *ivars, uint64_t nelems)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < nelems; i += (uint64_t)gridDim.x * kThreads)
        out[i] = snapshot_load(ivars + i);
}

}  // namespace sos

using namespace sos;

namespace {

unsigned *g_ticket = nullptr;

template <class A, bool UL>
int launch(char *dst, const char *src, const PsPlan &p, uint64_t *sig, uint64_t value, int sig_op, unsigned *ticket,
           hipStream_t st)
{
    hipLaunchKernelGGL((k_put_signal<A, UL>), dim3(p.grid), dim3(kThreads), 0, st, dst, src, p, sig, value, sig_op,
                       ticket);
    return hip_ok(hipGetLastError());
}

template <class T> int snapshot(void *out, const void *ivars, size_t nelems, hipStream_t st)
{
    const size_t wgs = (nelems + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((k_sync_snapshot<T>), dim3((unsigned)(wgs < kPsMaxGrid ? wgs : kPsMaxGrid)), dim3(kThreads), 0,
                       st, (T *)out, (const T *)ivars, (uint64_t)nelems);
    return hip_ok(hipGetLastError());
}

}  // namespace

extern "C" int sosx_put_signal(void *target, const void *source, size_t nbytes, uint64_t *sig_addr, uint64_t signal,
                               int sig_op, void *stream)
{
    return sosx_put_signal_on(target, source, nbytes, sig_addr, signal, sig_op, nullptr, stream);
}

// The same launch counting arrivals on `ticket`, a zeroed device word the caller owns
// (a context's: launches on different streams must not share one), or on the library's
// own when null.
extern "C" int sosx_put_signal_on(void *target, const void *source, size_t nbytes, uint64_t *sig_addr, uint64_t signal,
                                  int sig_op, unsigned *ticket, void *stream)
{
    // every argument is checked before any device work
    if (!sig_addr || (uintptr_t)sig_addr % sizeof(uint64_t)) return SOSX_ERR_ARG;
    if (sig_op != SOSX_SIGNAL_SET && sig_op != SOSX_SIGNAL_ADD) return SOSX_ERR_ARG;
    if (nbytes && (!target || !source)) return SOSX_ERR_ARG;
    if (nbytes > SIZE_MAX / 2) return SOSX_ERR_ARG;
    if (!ticket && !g_ticket) {
        if (hipMalloc((void **)&g_ticket, sizeof(unsigned)) != hipSuccess) {
            g_ticket = nullptr;
            return SOSX_ERR_HIP;
        }
        if (hipMemset(g_ticket, 0, sizeof(unsigned)) != hipSuccess) return SOSX_ERR_HIP;
    }
    if (!ticket) ticket = g_ticket;
    const PsPlan p = ps_plan((uintptr_t)target, (uintptr_t)source, nbytes);
    char *d = (char *)target;
    const char *s = (const char *)source;
    hipStream_t st = as_stream(stream);
    if (p.unaligned_loads) return launch<u32x4, true>(d, s, p, sig_addr, signal, sig_op, ticket, st);
    switch (p.width) {
        case 16: return launch<u32x4, false>(d, s, p, sig_addr, signal, sig_op, ticket, st);
        case 8: return launch<uint64_t, false>(d, s, p, sig_addr, signal, sig_op, ticket, st);
        case 4: return launch<uint32_t, false>(d, s, p, sig_addr, signal, sig_op, ticket, st);
        case 2: return launch<uint16_t, false>(d, s, p, sig_addr, signal, sig_op, ticket, st);
        case 1: return launch<uint8_t, false>(d, s, p, sig_addr, signal, sig_op, ticket, st);
        default: return SOSX_ERR_ARG;
    }
}

extern "C" int sosx_put_signal_plan(uintptr_t target, uintptr_t source, size_t nbytes, long long out[8])
{
    if (!out || nbytes > SIZE_MAX / 2) return SOSX_ERR_ARG;
    const PsPlan p = ps_plan(target, source, nbytes);
    out[0] = p.width;
    out[1] = p.unaligned_loads;
    out[2] = (long long)p.head;
    out[3] = (long long)p.units;
    out[4] = (long long)p.tail;
    out[5] = (long long)p.tiles;
    out[6] = p.grid;
    out[7] = kPsMaxGrid;
    return SOSX_OK;
}

extern "C" void *sosx_put_signal_ticket(void) { return g_ticket; }

extern "C" void sosx_put_signal_release(void)
{
    if (g_ticket) (void)hipFree(g_ticket);
    g_ticket = nullptr;
}

extern "C" int sosx_sync_snapshot(void *out, const void *ivars, size_t nelems, size_t width, void *stream)
{
    // every argument is checked before any device work
    if (width != 2 && width != 4 && width != 8) return SOSX_ERR_ARG;
    if (!nelems) return SOSX_OK;
    if (!out || !ivars || (uintptr_t)out % width || (uintptr_t)ivars % width) return SOSX_ERR_ARG;
    if (nelems > SIZE_MAX / 16) return SOSX_ERR_ARG;
    switch (width) {
        case 2: return snapshot<uint16_t>(out, ivars, nelems, as_stream(stream));
        case 4: return snapshot<uint32_t>(out, ivars, nelems, as_stream(stream));
        default: return snapshot<uint64_t>(out, ivars, nelems, as_stream(stream));
    }
}
