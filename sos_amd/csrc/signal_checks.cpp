// signal_checks.cpp -- what put-with-signal and the point-to-point waits decide on plain
// data: the argument checks (sos_put_signal_check, sos_sync_check) over the layout struct
// of sos_rma_check, and the comparison of a wait or test over a snapshot of its ivars
// (sos_sync_eval).  No HIP and no runtime state: the file compiles with a plain C++
// compiler, so tests/sync_eval_harness.cpp runs all of it as a program of its own.
#include <stdio.h>
#include <string.h>

#include "api_internal.h"

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

#define REFUSE(code, ...)                            \
    do {                                             \
        if (msg && n) snprintf(msg, n, __VA_ARGS__); \
        return code;                                 \
    } while (0)

namespace {

// SHMEM_ERR_CHECK_SYMMETRIC(ptr, len): nothing to check for len == 0
int symmetric(const sos_rma_layout *l, const char *name, const void *ptr, size_t len, const sos_rma_region **out,
              char *msg, size_t n)
{
    *out = nullptr;
    if (!len) return SOS_RMA_OK;
    const uintptr_t p = (uintptr_t)ptr;
    const sos_rma_region *reg = rma_find_region(l, p);
    if (!reg) REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\" is not symmetric (%p)", name, ptr);
    if (len > reg->size - (p - reg->base))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\" [%p..%p) exceeds %s [%p..%p)", name, ptr,
               (const void *)(p + len), rma_region_name(reg->kind), (const void *)reg->base,
               (const void *)(reg->base + reg->size));
    *out = reg;
    return SOS_RMA_OK;
}

// SHMEM_ERR_CHECK_OVERLAP(ptr1, ptr2, size1, size2, 0, 1): the lower extent may not reach
// the higher pointer; the message names ptr1 (src/shmem_internal.h:319-336)
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

bool mul_fits(size_t a, size_t b, size_t *out)
{
    if (b && a > (SIZE_MAX / 32) / b) return false;
    *out = a * b;
    return true;
}

}  // namespace

extern "C" int sos_put_signal_check(const sos_rma_layout *l, const sos_put_signal_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    int rc;
    if (!l->initialized) REFUSE(SOS_RMA_NOT_INITIALIZED, "library not initialized");
    if (op->pe < 0 || op->pe >= l->n_pes) REFUSE(SOS_RMA_BAD_PE, "PE argument (%d) is invalid", op->pe);
    size_t bytes = 0;
    if (!mul_fits(op->nelems, op->type_size, &bytes))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"target\": extent overflows size_t");
    const sos_rma_region *treg = nullptr, *sreg = nullptr;
    if ((rc = symmetric(l, "target", op->target, bytes, &treg, msg, n))) return rc;
    if (op->nelems > 0 && !op->source) REFUSE(SOS_RMA_NULL_LOCAL, "Argument \"source\" is NULL");
    if (op->pe == l->my_pe && (rc = overlap("target", op->target, bytes, op->sig_addr, sizeof(uint64_t), msg, n)))
        return rc;
    if (op->sig_op != 0 && op->sig_op != 1)
        REFUSE(SOS_SIG_BAD_OP, "Argument \"sig_op\", invalid atomic operation for signal (%d)", op->sig_op);
    // this library's own
    if ((rc = symmetric(l, "sig_addr", op->sig_addr, sizeof(uint64_t), &sreg, msg, n))) return rc;
    if ((uintptr_t)op->sig_addr % sizeof(uint64_t))
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Argument \"sig_addr\" (%p) must be aligned to 8 bytes", op->sig_addr);
    const size_t ts = op->type_size;
    if (ts != 1 && ts != 2 && ts != 4 && ts != 8 && ts != 16)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "element size %zu is not 1, 2, 4, 8 or 16", ts);
    if (bytes && ((uintptr_t)op->target % ts || (uintptr_t)op->source % ts))
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Arguments \"target\" (%p) and \"source\" (%p) must be aligned to the "
               "element size %zu", op->target, op->source, ts);
    if (op->pe == l->my_pe) return SOS_RMA_OK;
    const sos_rma_region *regs[2] = {treg, sreg};
    const void *ptrs[2] = {op->target, op->sig_addr};
    const char *names[2] = {"target", "sig_addr"};
    for (int k = 0; k < 2; ++k)
        if (regs[k] && regs[k]->kind != SOS_RMA_REGION_DEVICE_HEAP)
            REFUSE(SOS_RMA_PEER_NOT_DEVICE_HEAP, "Argument \"%s\" (%p) is in this PE's %s: put/get to another PE "
                   "(%d) needs the device symmetric heap (shmemx_malloc_device), the only memory mapped across PEs",
                   names[k], ptrs[k], rma_region_name(regs[k]->kind), op->pe);
    if (!l->mapped)
        REFUSE(SOS_RMA_NO_PATH, "No path to peer (PE %d's device heap is not mapped: SHMEMX_TRANSPORT=p2p or "
               "both maps it)", op->pe);
    return SOS_RMA_OK;
}

extern "C" int sos_sync_check(const sos_rma_layout *l, const sos_sync_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    int rc;
    if (!l->initialized) REFUSE(SOS_RMA_NOT_INITIALIZED, "library not initialized");
    const size_t ts = op->type_size;
    const char *name = op->kind == SOS_SYNC_ONE ? "ivar" : "ivars";
    // SOS checks the first ivar (sizeof(TYPE)); the probes here read all nelems of them, so
    // the whole array must lie in one region
    size_t bytes = 0;
    if (!mul_fits(op->nelems ? op->nelems : 1, ts, &bytes))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\": extent overflows size_t", name);
    const sos_rma_region *reg = nullptr;
    if ((rc = symmetric(l, name, op->ivars, bytes, &reg, msg, n))) return rc;
    if (op->kind != SOS_SYNC_ONE) {
        const size_t vb = ts * op->nelems, sb = sizeof(int) * op->nelems, ib = sizeof(size_t) * op->nelems;
        if (op->kind == SOS_SYNC_SOME && (rc = overlap("indices", op->indices, ib, op->status, sb, msg, n))) return rc;
        if ((rc = overlap(name, op->ivars, vb, op->status, sb, msg, n))) return rc;
        if (op->kind == SOS_SYNC_SOME && (rc = overlap(name, op->ivars, vb, op->indices, ib, msg, n))) return rc;
    }
    if (op->cmp < 1 || op->cmp > 6)
        REFUSE(SOS_SYNC_BAD_CMP, "Argument \"cmp\", invalid comparison operation (%d)", op->cmp);
    // this library's own
    if (ts != 2 && ts != 4 && ts != 8) REFUSE(SOS_RMA_BAD_TYPE_SIZE, "element size %zu is not 2, 4 or 8", ts);
    if ((uintptr_t)op->ivars % ts)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Argument \"%s\" (%p) must be aligned to the element size %zu", name,
               op->ivars, ts);
    if (op->kind == SOS_SYNC_SOME && op->nelems && !op->indices)
        REFUSE(SOS_RMA_NULL_LOCAL, "Argument \"indices\" is NULL");
    return SOS_RMA_OK;
}

#undef REFUSE

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
