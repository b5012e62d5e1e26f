// amo.cpp -- atomic memory operations on the symmetric heaps: the generic entry behind
// shmem_<T>_atomic_* and their deprecated and nbi forms (amo_gen.cpp).
//
// SOS's checks in SOS's order (src/atomic_c.c4:226-560: initialized, PE, symmetric over
// sizeof(TYPE)) as one function of plain data (sos_amo_check) over the layout struct of
// sos_rma_check; the entry raises what it refuses, translates the target as put / get do
// (translate, rma.cpp) and runs the operation:
//
//  * a target a kernel can reach -- any device-heap word, and for pe == my_pe the host
//    heap or a registered data segment (device_view) -- gets one launch of sosx_amo
//    (amo.hip) on the stream of the call's context (SHMEM_CTX_DEFAULT's, the library
//    stream, for the plain forms): one system-scope read-modify-write;
//  * a target in this PE's own pageable memory (static data under SHMEMX_REGISTER_DATA=0)
//    is memory only this process can address: the stream is completed, then the host does
//    the operation with the compiler's __atomic builtins;
//  * completion: the non-fetching forms only enqueue and complete at shmem_quiet /
//    shmem_fence / any barrier or sync, which complete the stream with a system-scope
//    release; the blocking fetching forms have the kernel store the old value into a
//    pinned host word the library owns, complete the stream (sync_system) and read it;
//    the nbi fetching forms enqueue, the kernel storing the old value into the program's
//    `fetch` where a kernel can reach it, else into a slot of a small device ring that a
//    copy on the same stream carries to `fetch` -- there no later than the next quiet;
//  * visibility, consumer half: a fetching operation on a peer's heap reads it, and
//    follows the acquire a wait may have left owed (before_peer_read, as get does).
//
// There is no wait on memory in this file: no spin in a kernel, no host polling loop.  The
// point-to-point waits (shmem_wait_until, shmem_test, shmem_signal_wait_until) are
// signal.cpp's: host-driven probes under a wall-clock bound, never a spin on the GPU.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "api_internal.h"
#include "runtime.h"
#include "sosx.h"

using namespace sosrt;

extern "C" int sos_amo_check(const sos_rma_layout *l, const sos_amo_op *op, char *msg, size_t n)
{
#define REFUSE(code, ...)                \
    do {                                 \
        if (msg && n) snprintf(msg, n, __VA_ARGS__); \
        return code;                     \
    } while (0)
    if (msg && n) msg[0] = 0;
    if (!l->initialized) REFUSE(SOS_RMA_NOT_INITIALIZED, "library not initialized");
    if (op->pe < 0 || op->pe >= l->n_pes) REFUSE(SOS_RMA_BAD_PE, "PE argument (%d) is invalid", op->pe);
    // SHMEM_ERR_CHECK_SYMMETRIC(target, sizeof(TYPE))
    const size_t ts = op->type_size;
    const uintptr_t t = (uintptr_t)op->target;
    const sos_rma_region *reg = rma_find_region(l, t);
    if (!reg) REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"target\" is not symmetric (%p)", op->target);
    if (ts > reg->size - (t - reg->base))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"target\" [%p..%p) exceeds %s [%p..%p)", op->target,
               (const void *)(t + ts), rma_region_name(reg->kind), (const void *)reg->base,
               (const void *)(reg->base + reg->size));
    if (ts != 4 && ts != 8) REFUSE(SOS_RMA_BAD_TYPE_SIZE, "element size %zu is not 4 or 8", ts);
    if (t % ts)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Argument \"target\" (%p) must be aligned to the element size %zu",
               op->target, ts);
    if (op->nbi) {
        if (!op->fetch) REFUSE(SOS_AMO_NULL_FETCH, "Argument \"fetch\" is NULL");
        if ((uintptr_t)op->fetch % ts)
            REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Argument \"fetch\" (%p) must be aligned to the element size %zu",
                   op->fetch, ts);
    }
    if (op->pe == l->my_pe) return SOS_RMA_OK;
    if (reg->kind != SOS_RMA_REGION_DEVICE_HEAP)
        REFUSE(SOS_RMA_PEER_NOT_DEVICE_HEAP, "Argument \"%s\" (%p) is in this PE's %s: put/get to another PE "
               "(%d) needs the device symmetric heap (shmemx_malloc_device), the only memory mapped across PEs",
               "target", op->target, rma_region_name(reg->kind), op->pe);
    if (!l->mapped)
        REFUSE(SOS_RMA_NO_PATH, "No path to peer (PE %d's device heap is not mapped: SHMEMX_TRANSPORT=p2p or "
               "both maps it)", op->pe);
    return SOS_RMA_OK;
#undef REFUSE
}

namespace {

constexpr unsigned kRingSlots = 64;  // nbi results on their way to pageable memory

// The ring of nbi results is the context's (Ctx::amo_ring): a fetching nbi atomic on
// context A is filled by A's quiet.  The blocking forms' word is shared: they complete
// their stream before they return, and the library is not thread-multiple.
struct AmoState {
    uint64_t *result = nullptr;      // pinned host word: a blocking form's old value
    uint64_t *result_dev = nullptr;  // its device view
};

AmoState &amo()
{
    static AmoState a;
    return a;
}

template <class T> T host_rmw(int op, T *p, T v, T c)
{
    switch (op) {
        case SOSX_AMO_FETCH: return __atomic_load_n(p, __ATOMIC_SEQ_CST);
        case SOSX_AMO_SET:
        case SOSX_AMO_SWAP: return __atomic_exchange_n(p, v, __ATOMIC_SEQ_CST);
        case SOSX_AMO_CSWAP:
            __atomic_compare_exchange_n(p, &c, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
            return c;  // the word's value either way
        case SOSX_AMO_ADD: return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST);
        case SOSX_AMO_AND: return __atomic_fetch_and(p, v, __ATOMIC_SEQ_CST);
        case SOSX_AMO_OR: return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST);
        default: return __atomic_fetch_xor(p, v, __ATOMIC_SEQ_CST);
    }
}

}  // namespace

void sosrt::amo_release()
{
    AmoState &a = amo();
    if (a.result) (void)hipHostFree(a.result);
    a = AmoState();
    Ctx &d = st().def_ctx;
    if (d.amo_ring) (void)hipFree(d.amo_ring);
    d.amo_ring = nullptr;
    d.amo_ring_used = 0;
}

void sosrt::amo_on(Ctx &cx, int op, void *target, const void *value, const void *cond, void *fetch_out, int want_old,
                   size_t type_size, int is_float, int pe, int nbi, const char *fn)
{
    State &s = st();
    {
        RmaLayout lay;
        rma_layout_now(lay);
        const sos_amo_op aop = {target, fetch_out, type_size, pe, nbi};
        char msg[512];
        if (sos_amo_check(&lay.l, &aop, msg, sizeof(msg)) != SOS_RMA_OK) raise_error("%s: %s", fn, msg);
    }
    if (op < SOSX_AMO_SET || op > SOSX_AMO_XOR ||
        (is_float && op != SOSX_AMO_SET && op != SOSX_AMO_FETCH && op != SOSX_AMO_SWAP))
        raise_error("%s: atomic operation %d is not defined on this type", fn, op);
    ++cx.enqueued;
    const size_t ts = type_size;
    uint64_t v = 0, c = 0;
    if (value) memcpy(&v, value, ts);
    if (cond) memcpy(&c, cond, ts);
    char *t = translate(target, pe);
    // the device heap is its own device view on every PE that maps it
    char *tdev = s.dev_heap.contains(target, ts) ? t : device_view(t, ts);
    if (!tdev) {
        // this PE's own pageable memory (the checks let only pe == my_pe come here): after
        // what the stream still has queued, the host does it
        hip_check(sync_system(cx), fn);
        const uint64_t old = ts == 4 ? host_rmw<uint32_t>(op, (uint32_t *)t, (uint32_t)v, (uint32_t)c)
                                     : host_rmw<uint64_t>(op, (uint64_t *)t, v, c);
        if (want_old) memcpy(fetch_out, &old, ts);
        return;
    }
    AmoState &a = amo();
    if (!want_old) {
        const int rc = sosx_amo(op, tdev, v, c, nullptr, ts, is_float, cx.stream);
        if (rc != SOSX_OK) raise_error("%s: atomic launch failed (%d)", fn, rc);
        return;
    }
    before_peer_read(cx, pe, fn);
    if (!nbi) {
        if (!a.result) {
            hip_check(hipHostMalloc((void **)&a.result, sizeof(uint64_t), hipHostMallocDefault), "hipHostMalloc(amo)");
            hip_check(hipHostGetDevicePointer((void **)&a.result_dev, a.result, 0), "hipHostGetDevicePointer(amo)");
        }
        const int rc = sosx_amo(op, tdev, v, c, a.result_dev, ts, is_float, cx.stream);
        if (rc != SOSX_OK) raise_error("%s: atomic launch failed (%d)", fn, rc);
        hip_check(sync_system(cx), fn);
        memcpy(fetch_out, a.result, ts);
        return;
    }
    if (char *fdev = device_view(fetch_out, ts)) {
        const int rc = sosx_amo(op, tdev, v, c, fdev, ts, is_float, cx.stream);
        if (rc != SOSX_OK) raise_error("%s: atomic launch failed (%d)", fn, rc);
        return;
    }
    // pageable `fetch`: a ring slot, then a copy on the same stream
    if (!cx.amo_ring) hip_check(hipMalloc((void **)&cx.amo_ring, kRingSlots * sizeof(uint64_t)), "hipMalloc(amo ring)");
    if (cx.amo_ring_used == kRingSlots) {
        hip_check(sync_system(cx), fn);
        cx.amo_ring_used = 0;
    }
    uint64_t *slot = cx.amo_ring + cx.amo_ring_used++;
    const int rc = sosx_amo(op, tdev, v, c, slot, ts, is_float, cx.stream);
    if (rc != SOSX_OK) raise_error("%s: atomic launch failed (%d)", fn, rc);
    hip_check(release_system(cx), fn);  // the copy engine reads HBM
    hip_check(hipMemcpyAsync(fetch_out, slot, ts, hipMemcpyDeviceToHost, cx.stream), fn);
}

extern "C" void sos_api_amo(int op, void *target, const void *value, const void *cond, void *fetch_out,
                            int want_old, size_t type_size, int is_float, int pe, int nbi, const char *fn)
{
    amo_on(default_ctx(), op, target, value, cond, fetch_out, want_old, type_size, is_float, pe, nbi, fn);
}

extern "C" void sos_api_ctx_amo(shmem_ctx_t ctx, int op, void *target, const void *value, const void *cond,
                                void *fetch_out, int want_old, size_t type_size, int is_float, int pe, int nbi,
                                const char *fn)
{
    Ctx &cx = ctx_checked(ctx, &pe, fn);
    amo_on(cx, op, target, value, cond, fetch_out, want_old, type_size, is_float, pe, nbi, fn);
}
