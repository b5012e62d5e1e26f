// onesided_checks.cpp -- what the one-sided layer decides on plain data (onesided_checks.h):
// the argument checks of put / get, the atomics, put-with-signal, the waits and tests, the
// locks and the contexts, the comparison of a wait or test over a snapshot of its ivars, and
// the texts of the two ways a lock call can end the job.  No HIP and no runtime state: the
// file compiles with a plain C++ compiler, so the harnesses under tests/ run all of it as
// programs of their own; rma.cpp, amo.cpp, signal.cpp, lock.cpp and ctx.cpp build the input
// from the runtime state and raise what is refused here.
//
// Every rule is written once, as a step below; a check is the ordered list of the steps that
// SOS's macros prescribe for its family (SOS's refusals in SOS's order), then this library's
// own.  The order of the steps within a check is behaviour.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "shmem.h"
#include "onesided_checks.h"

namespace sosrt {

const sos_rma_region *rma_find_region(const sos_rma_layout *l, uintptr_t p)
{
    for (int i = 0; i < l->nregions; ++i)
        if (p >= l->regions[i].base && p - l->regions[i].base < l->regions[i].size) return &l->regions[i];
    return nullptr;
}

const char *rma_region_name(int kind)
{
    return kind == SOS_RMA_REGION_HOST_HEAP ? "sym. heap region"
           : kind == SOS_RMA_REGION_DEVICE_HEAP ? "device sym. heap region"
           : kind == SOS_RMA_REGION_DATA ? "sym. data region" : "device allocation";
}

}  // namespace sosrt

using namespace sosrt;

#define REFUSE(code, ...) do { if (msg && n) snprintf(msg, n, __VA_ARGS__); return code; } while (0)
// one step of a check: its refusal is the check's
#define STEP(call) do { if (const int rc_ = (call)) return rc_; } while (0)
#define NEEDS_DEVICE_HEAP "needs the device symmetric heap (shmemx_malloc_device), the only memory mapped across PEs"

namespace {  // the steps

// SHMEM_ERR_CHECK_PE over [0, size)
int pe_in_range(int pe, int size, char *msg, size_t n)
{
    if (pe < 0 || pe >= size) REFUSE(SOS_RMA_BAD_PE, "PE argument (%d) is invalid", pe);
    return SOS_RMA_OK;
}

// SHMEM_ERR_CHECK_INITIALIZED, then SHMEM_ERR_CHECK_PE (pe == NULL: a call without one)
int initialized(const sos_rma_layout *l, const int *pe, char *msg, size_t n)
{
    if (!l->initialized) REFUSE(SOS_RMA_NOT_INITIALIZED, "library not initialized");
    return pe ? pe_in_range(*pe, l->n_pes, msg, n) : SOS_RMA_OK;
}

// A length in bytes that was computed without overflow, or fits == false and bytes == 0.
struct Extent {
    size_t bytes;
    bool fits;
};

// count * step + extra where that is at most SIZE_MAX / 32
Extent extent(size_t count, size_t step, size_t extra)
{
    const size_t cap = SIZE_MAX / 32;
    if (step && count > cap / step) return {0, false};
    if (extra > cap - count * step) return {0, false};
    return {count * step + extra, true};
}

int fits(const char *name, Extent e, char *msg, size_t n)
{
    if (!e.fits) REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\": extent overflows size_t", name);
    return SOS_RMA_OK;
}

// SHMEM_ERR_CHECK_SYMMETRIC(ptr, len): the whole extent lies in one region, *out
int symmetric(const sos_rma_layout *l, const char *name, const void *ptr, Extent len, const sos_rma_region **out,
              char *msg, size_t n)
{
    const uintptr_t p = (uintptr_t)ptr;
    const sos_rma_region *reg = *out = rma_find_region(l, p);
    if (!reg) REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\" is not symmetric (%p)", name, ptr);
    if (!len.fits || len.bytes > reg->size - (p - reg->base))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\" [%p..%p) exceeds %s [%p..%p)", name, ptr,
               (const void *)(p + len.bytes), rma_region_name(reg->kind), (const void *)reg->base,
               (const void *)(reg->base + reg->size));
    return SOS_RMA_OK;
}

// SHMEM_ERR_CHECK_NULL
int not_null(const char *name, const void *ptr, int code, char *msg, size_t n)
{
    if (!ptr) REFUSE(code, "Argument \"%s\" is NULL", name);
    return SOS_RMA_OK;
}

// SHMEM_ERR_CHECK_OVERLAP(ptr1, ptr2, size1, size2, 0, 1): the lower extent may not reach
// the higher pointer -- complete overlap is not allowed either; the message names ptr1
// (src/shmem_internal.h:319-336)
int overlap(const char *name1, const void *p1, size_t size1, const void *p2, size_t size2, char *msg, size_t n)
{
    const char *a = (const char *)p1, *b = (const char *)p2;
    if (!a || !b) return SOS_RMA_OK;  // an absent status or indices overlaps nothing
    const char *lo = a > b ? b : a, *hi = a > b ? a : b;
    const size_t sz_lo = a > b ? size2 : size1;
    if ((uintptr_t)lo + sz_lo > (uintptr_t)hi)
        REFUSE(SOS_RMA_OVERLAP, "Argument \"%s\" [%p..%p) overlaps argument (%p)", name1, (const void *)lo,
               (const void *)(lo + sz_lo), (const void *)hi);
    return SOS_RMA_OK;
}

// the element size is one of the powers of two in `mask`, which `list` spells out
int size_one_of(size_t ts, size_t mask, const char *list, char *msg, size_t n)
{
    if ((ts & (ts - 1)) || !(ts & mask)) REFUSE(SOS_RMA_BAD_TYPE_SIZE, "element size %zu is not %s", ts, list);
    return SOS_RMA_OK;
}

// aligned to `size`: the call's element size, or a fixed number of bytes
int aligned(const char *name, const void *ptr, size_t size, bool element, char *msg, size_t n)
{
    if ((uintptr_t)ptr % size)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Argument \"%s\" (%p) must be aligned to %s%zu%s", name, ptr,
               element ? "the element size " : "", size, element ? "" : " bytes");
    return SOS_RMA_OK;
}

// both sides of a copy
int aligned_pair(const void *target, const void *source, size_t ts, char *msg, size_t n)
{
    if ((uintptr_t)target % ts || (uintptr_t)source % ts)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Arguments \"target\" (%p) and \"source\" (%p) must be aligned to the "
               "element size %zu", target, source, ts);
    return SOS_RMA_OK;
}

// This library's own: another PE reaches the device heap only (every argument, in the
// call's order; reg == NULL: an argument of no bytes), and only where it is mapped.
struct Remote {
    const char *name;
    const void *ptr;
    const sos_rma_region *reg;
};
int peer_reach(const sos_rma_layout *l, int pe, std::initializer_list<Remote> args, char *msg, size_t n)
{
    if (pe == l->my_pe) return SOS_RMA_OK;
    for (const Remote &a : args)
        if (a.reg && a.reg->kind != SOS_RMA_REGION_DEVICE_HEAP)
            REFUSE(SOS_RMA_PEER_NOT_DEVICE_HEAP, "Argument \"%s\" (%p) is in this PE's %s: put/get to another PE "
                   "(%d) " NEEDS_DEVICE_HEAP, a.name, a.ptr, rma_region_name(a.reg->kind), pe);
    if (!l->mapped)
        REFUSE(SOS_RMA_NO_PATH, "No path to peer (PE %d's device heap is not mapped: SHMEMX_TRANSPORT=p2p or "
               "both maps it)", pe);
    return SOS_RMA_OK;
}

}  // namespace

// ---- put / get: SOS's order (src/data_c.c4:300-680) ---------------------------------------
extern "C" int sos_rma_check(const sos_rma_layout *l, const sos_rma_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    const char *rname = op->put ? "target" : "source", *lname = op->put ? "source" : "target";
    // the strides as SOS's prototypes name them: tst is the target's, sst the source's
    const ptrdiff_t strides[2] = {op->put ? op->remote_stride : op->local_stride,
                                  op->put ? op->local_stride : op->remote_stride};
    const char *const stride_names[2] = {"tst", "sst"};
    STEP(initialized(l, &op->pe, msg, n));
    const size_t ts = op->type_size;
    STEP(size_one_of(ts, 1 | 2 | 4 | 8 | 16, "1, 2, 4, 8 or 16", msg, n));
    for (int k = 0; k < 2 && op->strided; ++k)  // SHMEM_ERR_CHECK_POSITIVE(tst), then (sst)
        if (strides[k] <= 0)
            REFUSE(SOS_RMA_NOT_POSITIVE, "Argument %s must be positive (%ld)", stride_names[k], (long)strides[k]);
    const bool empty = op->bsize == 0 || op->nblocks == 0;
    // elements spanned by nblocks blocks of bsize at a stride (>= 0), then bytes
    auto span = [&](ptrdiff_t stride) {
        Extent e = extent(op->nblocks - 1, stride > 0 ? (size_t)stride : 0, op->bsize);
        e.bytes *= ts;
        return e;
    };
    Extent rext = {0, true};
    const sos_rma_region *reg = nullptr;
    if (!empty) {
        // SHMEM_ERR_CHECK_SYMMETRIC over the remote side's whole extent
        rext = span(op->remote_stride);
        STEP(symmetric(l, rname, op->remote, rext, &reg, msg, n));
        STEP(not_null(lname, op->local, SOS_RMA_NULL_LOCAL, msg, n));
    }
    for (int k = 0; k < 2; ++k)  // SHMEM_ERR_CHECK_STRIDE_GTE_BSIZE(tst), then (sst)
        if (strides[k] < 0 || (size_t)strides[k] < op->bsize)
            REFUSE(SOS_RMA_STRIDE_LT_BSIZE, "Stride argument \"%s\" (%zd), is less than block size %zu",
                   stride_names[k], strides[k], op->bsize);
    if (empty) return SOS_RMA_OK;
    const Extent lext = span(op->local_stride);
    STEP(fits(lname, lext, msg, n));
    STEP(aligned_pair(op->put ? op->remote : op->local, op->put ? op->local : op->remote, ts, msg, n));
    // SHMEM_ERR_CHECK_OVERLAP, for the calling PE itself
    if (op->pe == l->my_pe) STEP(overlap("target", op->remote, rext.bytes, op->local, lext.bytes, msg, n));
    return peer_reach(l, op->pe, {{rname, op->remote, reg}}, msg, n);
}

// ---- atomics: SOS's order (src/atomic_c.c4:226-560: initialized, PE, symmetric over
// sizeof(TYPE)), then this library's own ----------------------------------------------------
extern "C" int sos_amo_check(const sos_rma_layout *l, const sos_amo_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    STEP(initialized(l, &op->pe, msg, n));
    // SHMEM_ERR_CHECK_SYMMETRIC(target, sizeof(TYPE))
    const size_t ts = op->type_size;
    const sos_rma_region *reg = nullptr;
    STEP(symmetric(l, "target", op->target, {ts, true}, &reg, msg, n));
    STEP(size_one_of(ts, 4 | 8, "4 or 8", msg, n));
    STEP(aligned("target", op->target, ts, true, msg, n));
    if (op->nbi) {
        STEP(not_null("fetch", op->fetch, SOS_AMO_NULL_FETCH, msg, n));
        STEP(aligned("fetch", op->fetch, ts, true, msg, n));
    }
    return peer_reach(l, op->pe, {{"target", op->target, reg}}, msg, n);
}

// ---- put with signal: SOS's order (src/data_c.c4:691-699: initialized, PE, target
// symmetric, source NULL, overlap for pe == my_pe, sig_op), then this library's own --------
extern "C" int sos_put_signal_check(const sos_rma_layout *l, const sos_put_signal_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    STEP(initialized(l, &op->pe, msg, n));
    const Extent bytes = extent(op->nelems, op->type_size, 0);
    STEP(fits("target", bytes, msg, n));
    const sos_rma_region *treg = nullptr, *sreg = nullptr;
    // SHMEM_ERR_CHECK_SYMMETRIC(target, len): nothing to check for len == 0
    if (bytes.bytes) STEP(symmetric(l, "target", op->target, bytes, &treg, msg, n));
    if (op->nelems > 0) STEP(not_null("source", op->source, SOS_RMA_NULL_LOCAL, msg, n));
    if (op->pe == l->my_pe) STEP(overlap("target", op->target, bytes.bytes, op->sig_addr, sizeof(uint64_t), msg, n));
    if (op->sig_op != 0 && op->sig_op != 1)
        REFUSE(SOS_SIG_BAD_OP, "Argument \"sig_op\", invalid atomic operation for signal (%d)", op->sig_op);
    // this library's own
    STEP(symmetric(l, "sig_addr", op->sig_addr, {sizeof(uint64_t), true}, &sreg, msg, n));
    STEP(aligned("sig_addr", op->sig_addr, sizeof(uint64_t), false, msg, n));
    const size_t ts = op->type_size;
    STEP(size_one_of(ts, 1 | 2 | 4 | 8 | 16, "1, 2, 4, 8 or 16", msg, n));
    if (bytes.bytes) STEP(aligned_pair(op->target, op->source, ts, msg, n));
    return peer_reach(l, op->pe, {{"target", op->target, treg}, {"sig_addr", op->sig_addr, sreg}}, msg, n);
}

// ---- waits and tests: SOS's order (src/synchronization_c.c4: initialized, ivars symmetric,
// the overlaps, the comparison), then this library's own ------------------------------------
extern "C" int sos_sync_check(const sos_rma_layout *l, const sos_sync_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    STEP(initialized(l, nullptr, msg, n));
    const size_t ts = op->type_size;
    const char *name = op->kind == SOS_SYNC_ONE ? "ivar" : "ivars";
    // SOS checks the first ivar (sizeof(TYPE)); the probes here read all nelems of them, so
    // the whole array must lie in one region
    const Extent bytes = extent(op->nelems ? op->nelems : 1, ts, 0);
    STEP(fits(name, bytes, msg, n));
    const sos_rma_region *reg = nullptr;
    if (bytes.bytes) STEP(symmetric(l, name, op->ivars, bytes, &reg, msg, n));
    if (op->kind != SOS_SYNC_ONE) {
        const size_t vb = ts * op->nelems, sb = sizeof(int) * op->nelems, ib = sizeof(size_t) * op->nelems;
        if (op->kind == SOS_SYNC_SOME) STEP(overlap("indices", op->indices, ib, op->status, sb, msg, n));
        STEP(overlap(name, op->ivars, vb, op->status, sb, msg, n));
        if (op->kind == SOS_SYNC_SOME) STEP(overlap(name, op->ivars, vb, op->indices, ib, msg, n));
    }
    if (op->cmp < 1 || op->cmp > 6)
        REFUSE(SOS_SYNC_BAD_CMP, "Argument \"cmp\", invalid comparison operation (%d)", op->cmp);
    // this library's own
    STEP(size_one_of(ts, 2 | 4 | 8, "2, 4 or 8", msg, n));
    STEP(aligned(name, op->ivars, ts, true, msg, n));
    if (op->kind == SOS_SYNC_SOME && op->nelems) STEP(not_null("indices", op->indices, SOS_RMA_NULL_LOCAL, msg, n));
    return SOS_RMA_OK;
}

// ---- locks: SOS's order (src/lock_c.c:44-65): SHMEM_ERR_CHECK_INITIALIZED, then
// SHMEM_ERR_CHECK_SYMMETRIC(lock, sizeof(long)); then this library's own.  Nothing here
// depends on my_pe: PE 0, the home of `last`, refuses what every other PE refuses. ----------
extern "C" int sos_lock_check(const sos_rma_layout *l, const sos_lock_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    STEP(initialized(l, nullptr, msg, n));
    const sos_rma_region *reg = nullptr;
    STEP(symmetric(l, "lock", op->lock, {sizeof(long), true}, &reg, msg, n));
    // this library's own
    STEP(aligned("lock", op->lock, sizeof(long), false, msg, n));
    if (l->n_pes == 1) return SOS_RMA_OK;
    // peer_reach's two rules for a word that EVERY PE reaches, in the lock's own words
    if (reg->kind != SOS_RMA_REGION_DEVICE_HEAP)
        REFUSE(SOS_RMA_PEER_NOT_DEVICE_HEAP, "Argument \"lock\" (%p) is in this PE's %s: a lock shared by %d PEs "
               NEEDS_DEVICE_HEAP, op->lock, rma_region_name(reg->kind), l->n_pes);
    if (!l->mapped)
        REFUSE(SOS_RMA_NO_PATH, "No path to peer (the PEs' device heaps are not mapped: SHMEMX_TRANSPORT=p2p or "
               "both maps them)");
    return SOS_RMA_OK;
}

extern "C" void sos_lock_expiry_message(const char *fn, const void *lock, int awaited, uint32_t data, double seconds,
                                        char *msg, size_t n)
{
    if (!msg || !n) return;
    snprintf(msg, n, "%s: lock %p not %s after %.0f s (SHMEMX_P2P_TIMEOUT): awaited %s in this PE's data half, "
             "last value seen 0x%08x (next = %u, signal = %u)", fn, lock,
             awaited == SOS_LOCK_AWAIT_SIGNAL ? "granted" : "handed over", seconds,
             awaited == SOS_LOCK_AWAIT_SIGNAL ? "SIGNAL (bit 31) from the predecessor"
                                              : "NEXT (bits 0-30) from the successor",
             data, data & 0x7FFFFFFFu, data >> 31);
}

extern "C" void sos_lock_corrupt_message(const void *lock, int value, int n_pes, char *msg, size_t n)
{
    if (!msg || !n) return;
    snprintf(msg, n, "lock word at %p is not a lock (last/next = %d, n_pes = %d): was it zero-initialised?", lock,
             value, n_pes);
}

// ---- contexts: a handle is LOOKED UP in the table of live contexts and never dereferenced;
// then the call's `pe`, an index of the context's team (SOS: shmem_internal_team_pe before
// the checks, src/data_c.c4:829-835), becomes the world PE start + pe * stride -------------
extern "C" int sos_ctx_check(const sos_ctx_table *t, const void *handle, int *pe, int *index, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    if (index) *index = -1;
    if (!handle) REFUSE(SOS_CTX_INVALID, "Argument \"ctx\" is SHMEM_CTX_INVALID");
    const sos_ctx_entry *e = nullptr;
    for (int i = 0; i < t->nlive && !e; ++i)
        if (t->live[i].handle == handle) {
            e = &t->live[i];
            if (index) *index = i;
        }
    if (!e) {
        for (int i = 0; i < t->ndead; ++i)
            if (t->dead[i] == handle)
                REFUSE(SOS_CTX_DESTROYED, "Argument \"ctx\" (%p) is a context that was destroyed", handle);
        REFUSE(SOS_CTX_UNKNOWN, "Argument \"ctx\" (%p) is not a context of this library", handle);
    }
    if (!pe) return SOS_CTX_OK;
    STEP(pe_in_range(*pe, e->size, msg, n));
    *pe = e->start + *pe * e->stride;
    return SOS_CTX_OK;
}

extern "C" int sos_ctx_options_check(long options, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    const long known = SHMEM_CTX_PRIVATE | SHMEM_CTX_SERIALIZED | SHMEM_CTX_NOSTORE;
    if (options & ~known)
        REFUSE(SOS_CTX_BAD_OPTIONS, "Argument \"options\" (0x%lx) has bits outside SHMEM_CTX_PRIVATE | "
               "SHMEM_CTX_SERIALIZED | SHMEM_CTX_NOSTORE", (unsigned long)options);
    return SOS_CTX_OK;
}

extern "C" int sos_ctx_pool_size(const char *v, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    if (!v || !*v) return 3;
    char *end = nullptr;
    errno = 0;
    const long k = strtol(v, &end, 10);
    if (errno || *end || k < 1 || k > 31) REFUSE(-1, "SHMEMX_CTX_STREAMS=%s is not a number in 1..31", v);
    return (int)k;
}

extern "C" int sos_ctx_stream_slot(unsigned long created, int pool_size)
{
    return pool_size > 0 ? (int)(created % (unsigned long)pool_size) : 0;
}

#undef REFUSE
#undef STEP

// ---- the comparison of a wait or test -----------------------------------------------------
namespace {

template <class T> bool compare(int cmp, T a, T b)
{
    switch (cmp) {
        case 1: return a == b;  // SHMEM_CMP_EQ
        case 2: return a != b;  // SHMEM_CMP_NE
        case 3: return a > b;   // SHMEM_CMP_GT
        case 4: return a >= b;  // SHMEM_CMP_GE
        case 5: return a < b;   // SHMEM_CMP_LT
        default: return a <= b;  // SHMEM_CMP_LE
    }
}

template <class T> T word(const void *p, size_t i)
{
    T v;
    memcpy(&v, (const char *)p + i * sizeof(T), sizeof(T));
    return v;
}

template <class T>
int eval(const void *snap, size_t nelems, const int *status, int cmp, const void *value, int vector, int kind,
         size_t *index, size_t *indices, size_t *count)
{
    size_t live = 0, hold = 0, first = SIZE_MAX;
    for (size_t i = 0; i < nelems; ++i) {
        if (status && status[i]) continue;
        ++live;
        if (!compare<T>(cmp, word<T>(snap, i), word<T>(value, vector ? i : 0))) continue;
        if (first == SIZE_MAX) first = i;
        if (kind == SOS_SYNC_SOME && indices) indices[hold] = i;
        ++hold;
    }
    if (index) *index = kind == SOS_SYNC_ANY ? first : SIZE_MAX;
    if (count) *count = kind == SOS_SYNC_SOME ? hold : 0;
    if (!live) return 1;  // nothing to wait for
    return kind == SOS_SYNC_ONE || kind == SOS_SYNC_ALL ? hold == live : hold > 0;
}

}  // namespace

extern "C" int sos_sync_eval(const void *snapshot, size_t nelems, size_t width, int is_signed, const int *status,
                             int cmp, const void *value, int vector, int kind, size_t *index, size_t *indices,
                             size_t *count)
{
    if (cmp < 1 || cmp > 6 || kind < SOS_SYNC_ONE || kind > SOS_SYNC_SOME) return -1;
    if (nelems && (!snapshot || !value)) return -1;
    if (kind == SOS_SYNC_SOME && nelems && !indices) return -1;
    if (kind == SOS_SYNC_ONE && nelems != 1) return -1;
#define EVAL(T) eval<T>(snapshot, nelems, status, cmp, value, vector, kind, index, indices, count)
    switch (width) {
        case 2: return is_signed ? EVAL(int16_t) : EVAL(uint16_t);
        case 4: return is_signed ? EVAL(int32_t) : EVAL(uint32_t);
        case 8: return is_signed ? EVAL(int64_t) : EVAL(uint64_t);
        default: return -1;
    }
#undef EVAL
}
