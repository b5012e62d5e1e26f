// amo.cpp -- atomic memory operations on the symmetric heaps: the generic entry behind
// shmem_<T>_atomic_* and their deprecated and nbi forms (amo_gen.cpp).
//
// SOS's checks in SOS's order (src/atomic_c.c4:226-560: initialized, PE, symmetric over
// sizeof(TYPE)) are one function of plain data (sos_amo_check, onesided_checks.cpp); the
// entry raises what it refuses (checked), translates the target as put / get do (translate,
// onesided.cpp) and runs the operation:
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
//    pinned host word the library owns (Pinned, onesided.cpp), complete the stream
//    (sync_system) and read it;
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
#include <string.h>

#include "onesided.h"
#include "runtime.h"
#include "sosx.h"

using namespace sosrt;

namespace {

constexpr unsigned kRingSlots = 64;  // nbi results on their way to pageable memory

// The ring of nbi results is the context's (Ctx::amo_ring): a fetching nbi atomic on
// context A is filled by A's quiet.  The blocking forms' word is shared: they complete
// their stream before they return, and the library is not thread-multiple.
Pinned &result_word()  // a blocking form's old value
{
    static Pinned p;
    return p;
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
    result_word().release();
    Ctx &d = st().def_ctx;
    if (d.amo_ring) (void)hipFree(d.amo_ring);
    d.amo_ring = nullptr;
    d.amo_ring_used = 0;
}

void sosrt::amo_on(Ctx &cx, int op, void *target, const void *value, const void *cond, void *fetch_out, int want_old,
                   size_t type_size, int is_float, int pe, int nbi, const char *fn)
{
    State &s = st();
    checked(sos_amo_check, sos_amo_op{target, fetch_out, type_size, pe, nbi}, fn);
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
    // one launch of the operation; the old value, where wanted, goes to `old`
    auto launch = [&](void *old) {
        const int rc = sosx_amo(op, tdev, v, c, old, ts, is_float, cx.stream);
        if (rc != SOSX_OK) raise_error("%s: atomic launch failed (%d)", fn, rc);
    };
    if (!want_old) return launch(nullptr);
    before_peer_read(cx, pe, fn);
    if (!nbi) {
        Pinned &word = result_word();
        word.reserve(sizeof(uint64_t), cx.stream, "amo", fn);
        launch(word.dev);
        hip_check(sync_system(cx), fn);
        memcpy(fetch_out, word.host, ts);
        return;
    }
    if (char *fdev = device_view(fetch_out, ts)) return launch(fdev);
    // pageable `fetch`: a ring slot, then a copy on the same stream
    if (!cx.amo_ring) hip_check(hipMalloc((void **)&cx.amo_ring, kRingSlots * sizeof(uint64_t)), "hipMalloc(amo ring)");
    if (cx.amo_ring_used == kRingSlots) {
        hip_check(sync_system(cx), fn);
        cx.amo_ring_used = 0;
    }
    uint64_t *slot = cx.amo_ring + cx.amo_ring_used++;
    launch(slot);
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
