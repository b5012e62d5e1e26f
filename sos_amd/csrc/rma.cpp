// rma.cpp -- one-sided put / get on the device symmetric heap: the generic entries behind
// shmem_put / get / p / g / iput / iget, shmemx_ibput / ibget and shmem_ptr (rma_gen.cpp).
//
// SOS's checks in SOS's order (src/data_c.c4:300-680) as one function of plain data
// (sos_rma_check); the entries build its input from the runtime state, raise what it
// refuses, translate the remote address and move the bytes on the library stream:
//
//  * translation: a device-heap address belongs to PE `pe` at
//    peer_heap[pe] + (addr - peer_heap[my_pe]) (every PE maps every heap under
//    SHMEMX_TRANSPORT=p2p|both, ensure_device_heap); pe == my_pe needs no mapping and may
//    name any symmetric memory;
//  * contiguous forms: hipMemcpyAsync on the library stream behind a system-scope release
//    (the copy engine reads HBM), as sosx_memcpy orders its copy; the blocking forms then
//    complete the stream like every other call (sync_system);
//  * strided and block forms: sosx_block_strided_copy (blockcopy.hip); a side that a
//    kernel cannot reach (pageable host memory: the local side, or unregistered static
//    data as the remote side of a call to the calling PE itself) is packed into /
//    unpacked from stage() by a 2-D copy, which touches the blocks only;
//  * completion: the blocking forms return after sync_system(stream) -- local and remote
//    completion at once; the nbi forms only enqueue, and shmem_quiet / shmem_fence / every
//    barrier and sync complete the stream with a system-scope release;
//  * visibility, consumer half: a launch that reads a peer's heap follows an acquire
//    issued after the last wait for a peer (acquire_system; note_peer_read counts it);
//  * contexts: "the library stream" above is the stream of the context the call names --
//    SHMEM_CTX_DEFAULT for the plain forms -- with that context's release event, stage and
//    acquire flag (ctx.cpp).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "api_internal.h"
#include "runtime.h"
#include "shmemx.h"
#include "sosx.h"

using namespace sosrt;

extern "C" char __data_start[] __attribute__((weak));
extern "C" char _end[] __attribute__((weak));

// rma_find_region and rma_region_name live in signal_checks.cpp, the file without HIP

namespace {

// elements spanned by nblocks blocks of bsize at `stride` (>= 0); false if over size_t
bool extent_bytes(size_t bsize, size_t nblocks, ptrdiff_t stride, size_t ts, size_t *out)
{
    const size_t s = stride > 0 ? (size_t)stride : 0;
    if (s && nblocks - 1 > (SIZE_MAX / 32) / s) return false;
    const size_t span = (nblocks - 1) * s;
    if (bsize > SIZE_MAX / 32 - span) return false;
    *out = (span + bsize) * ts;
    return true;
}

}  // namespace

extern "C" int sos_rma_check(const sos_rma_layout *l, const sos_rma_op *op, char *msg, size_t n)
{
#define REFUSE(code, ...)                \
    do {                                 \
        if (msg && n) snprintf(msg, n, __VA_ARGS__); \
        return code;                     \
    } while (0)
    if (msg && n) msg[0] = 0;
    const char *rname = op->put ? "target" : "source", *lname = op->put ? "source" : "target";
    // the stride names as SOS's prototypes have them: tst is the target's
    const char *rsname = op->put ? "tst" : "sst", *lsname = op->put ? "sst" : "tst";
    if (!l->initialized) REFUSE(SOS_RMA_NOT_INITIALIZED, "library not initialized");
    if (op->pe < 0 || op->pe >= l->n_pes) REFUSE(SOS_RMA_BAD_PE, "PE argument (%d) is invalid", op->pe);
    const size_t ts = op->type_size;
    if (ts != 1 && ts != 2 && ts != 4 && ts != 8 && ts != 16)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "element size %zu is not 1, 2, 4, 8 or 16", ts);
    if (op->strided) {  // SHMEM_ERR_CHECK_POSITIVE(tst), then (sst)
        const ptrdiff_t tst = op->put ? op->remote_stride : op->local_stride;
        const ptrdiff_t sst = op->put ? op->local_stride : op->remote_stride;
        if (tst <= 0) REFUSE(SOS_RMA_NOT_POSITIVE, "Argument %s must be positive (%ld)", "tst", (long)tst);
        if (sst <= 0) REFUSE(SOS_RMA_NOT_POSITIVE, "Argument %s must be positive (%ld)", "sst", (long)sst);
    }
    const bool empty = op->bsize == 0 || op->nblocks == 0;
    size_t rext = 0, lext = 0;
    const sos_rma_region *reg = nullptr;
    if (!empty) {
        // SHMEM_ERR_CHECK_SYMMETRIC over the remote side's whole extent
        const uintptr_t r = (uintptr_t)op->remote;
        reg = rma_find_region(l, r);
        if (!reg) REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\" is not symmetric (%p)", rname, op->remote);
        if (!extent_bytes(op->bsize, op->nblocks, op->remote_stride, ts, &rext) ||
            rext > reg->size - (r - reg->base))
            REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\" [%p..%p) exceeds %s [%p..%p)", rname, op->remote,
                   (const void *)(r + rext), rma_region_name(reg->kind), (const void *)reg->base,
                   (const void *)(reg->base + reg->size));
        // SHMEM_ERR_CHECK_NULL
        if (!op->local) REFUSE(SOS_RMA_NULL_LOCAL, "Argument \"%s\" is NULL", lname);
    }
    // SHMEM_ERR_CHECK_STRIDE_GTE_BSIZE(tst), then (sst)
    for (int k = 0; k < 2; ++k) {
        const bool remote_first = op->put;  // tst first
        const bool remote = (k == 0) == remote_first;
        const ptrdiff_t s = remote ? op->remote_stride : op->local_stride;
        if (s < 0 || (size_t)s < op->bsize)
            REFUSE(SOS_RMA_STRIDE_LT_BSIZE, "Stride argument \"%s\" (%zd), is less than block size %zu",
                   remote ? rsname : lsname, s, op->bsize);
    }
    if (empty) return SOS_RMA_OK;
    if (!extent_bytes(op->bsize, op->nblocks, op->local_stride, ts, &lext))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"%s\": extent overflows size_t", lname);
    if ((uintptr_t)op->remote % ts || (uintptr_t)op->local % ts)
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Arguments \"target\" (%p) and \"source\" (%p) must be aligned to the "
               "element size %zu", op->put ? op->remote : op->local, op->put ? op->local : op->remote, ts);
    if (op->pe == l->my_pe) {
        // SHMEM_ERR_CHECK_OVERLAP, complete overlap not allowed
        const char *a = (const char *)op->remote, *b = (const char *)op->local;
        if (a < b + lext && b < a + rext) {
            const char *lo = a < b ? a : b, *hi = a < b ? b : a;
            REFUSE(SOS_RMA_OVERLAP, "Argument \"target\" [%p..%p) overlaps argument (%p)", (const void *)lo,
                   (const void *)(lo + (lo == a ? rext : lext)), (const void *)hi);
        }
        return SOS_RMA_OK;
    }
    if (reg->kind != SOS_RMA_REGION_DEVICE_HEAP)
        REFUSE(SOS_RMA_PEER_NOT_DEVICE_HEAP, "Argument \"%s\" (%p) is in this PE's %s: put/get to another PE "
               "(%d) needs the device symmetric heap (shmemx_malloc_device), the only memory mapped across PEs",
               rname, op->remote, rma_region_name(reg->kind), op->pe);
    if (!l->mapped)
        REFUSE(SOS_RMA_NO_PATH, "No path to peer (PE %d's device heap is not mapped: SHMEMX_TRANSPORT=p2p or "
               "both maps it)", op->pe);
    return SOS_RMA_OK;
#undef REFUSE
}

namespace {

bool heap_mapped(const State &s)
{
    if (!s.p2p_ready || s.peer_heap.size() != (size_t)s.n_pes) return false;
    for (char *b : s.peer_heap)
        if (!b) return false;
    return true;
}

}  // namespace

void sosrt::rma_layout_now(RmaLayout &out)
{
    State &s = st();
    auto add = [&](const void *b, size_t n, int kind) {
        if (b && n) out.regions.push_back({(uintptr_t)b, n, kind});
    };
    // the executable's data segment, as is_symmetric has it
    const char *data = __data_start && _end ? __data_start : nullptr;
    const size_t data_bytes = data ? (size_t)(_end - __data_start) : 0;
    add(s.dev_heap.base, s.dev_heap.size, SOS_RMA_REGION_DEVICE_HEAP);
    add(s.host_heap.base, s.host_heap.size, SOS_RMA_REGION_HOST_HEAP);
    add(data, data_bytes, SOS_RMA_REGION_DATA);
    for (auto &kv : s.dev_allocs) add(kv.first, kv.second, SOS_RMA_REGION_DEVICE_ALLOC);
    out.l = {s.initialized && !s.finalized, s.my_pe, s.n_pes, heap_mapped(s), (int)out.regions.size(),
             out.regions.data()};
}

namespace {

void checked(const sos_rma_op &op, const char *fn)
{
    RmaLayout lay;
    rma_layout_now(lay);
    char msg[512];
    if (sos_rma_check(&lay.l, &op, msg, sizeof(msg)) != SOS_RMA_OK) raise_error("%s: %s", fn, msg);
}

}  // namespace

// the remote side's address on this PE
char *sosrt::translate(const void *remote, int pe)
{
    State &s = st();
    if (pe == s.my_pe) return (char *)remote;
    return s.peer_heap[(size_t)pe] + ((const char *)remote - s.peer_heap[(size_t)s.my_pe]);
}

// Before a launch or copy that reads peer `pe`'s heap: the acquire a wait since the last
// one left owed, and the read counted.
void sosrt::before_peer_read(Ctx &c, int pe, const char *fn)
{
    if (pe == st().my_pe) return;
    if (c.acq_pending) hip_check(acquire_system(c), fn);  // on the stream that does the read
    note_peer_read(c, false);
}

// The address at which a kernel on this PE's GPU reaches the `bytes` bytes at p, or null
// where it cannot (pageable host memory, or an extent only partly registered with HIP,
// such as a data segment whose first page was rounded off).  Device memory is its own
// address; host memory that HIP allocated or registered is reached through the device
// pointer HIP reports for it (hipHostGetDevicePointer's), which need not equal p.
char *sosrt::device_view(const void *p, size_t bytes)
{
    if (is_device_ptr(p)) return (char *)p;
    hipPointerAttribute_t a, z;
    if (hipPointerGetAttributes(&a, p) != hipSuccess ||
        hipPointerGetAttributes(&z, (const char *)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    const bool host = a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged;
    if (!host || z.type != a.type || !a.devicePointer || !z.devicePointer) return nullptr;
    // one mapping over the whole extent
    if ((char *)z.devicePointer - (char *)a.devicePointer != (ptrdiff_t)(bytes - 1)) return nullptr;
    return (char *)a.devicePointer;
}

namespace {

void contiguous(Ctx &c, void *dst, const void *src, size_t bytes, int read_pe, bool nbi, const char *fn)
{
    if (!bytes) return;
    ++c.enqueued;
    before_peer_read(c, read_pe, fn);
    // the copy engine reads HBM: what the stream's kernels stored goes there first
    hip_check(release_system(c), fn);
    hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c.stream), fn);
    if (!nbi) hip_check(sync_system(c), fn);
}

size_t span_bytes(size_t bsize, size_t nblocks, ptrdiff_t stride, size_t ts)
{
    return ((nblocks - 1) * (size_t)stride + bsize) * ts;  // sos_rma_check bounded it
}

// dst/src with strides in elements; one of them is the remote side (translated).  EITHER
// side may be memory a kernel cannot reach: the local side may be any memory, and for
// pe == my_pe the remote side may be static data that is not registered with HIP
// (SHMEMX_REGISTER_DATA=0, a refused registration, the rounded-off first page).  Such a
// side is packed into / unpacked from stage() by a 2-D copy, which touches the blocks only.
void blocks(Ctx &c, char *dst, ptrdiff_t dstr, const char *src, ptrdiff_t sstr, size_t bsize, size_t nblocks,
            size_t ts, int read_pe, const char *fn)
{
    if (!bsize || !nblocks) return;
    ++c.enqueued;
    const size_t bbytes = bsize * ts;
    char *ddev = device_view(dst, span_bytes(bsize, nblocks, dstr, ts));
    const char *sdev = device_view(src, span_bytes(bsize, nblocks, sstr, ts));
    int rc = SOSX_OK;
    if (ddev && sdev) {
        before_peer_read(c, read_pe, fn);
        rc = sosx_block_strided_copy(ddev, dstr, sdev, sstr, bsize, nblocks, ts, c.stream);
    } else if (ddev) {
        // pageable source: pack the blocks into the stage, then the kernel
        char *stg = (char *)stage(c, bbytes * nblocks);
        hip_check(hipMemcpy2DAsync(stg, bbytes, src, (size_t)sstr * ts, bbytes, nblocks, hipMemcpyHostToDevice,
                                   c.stream), fn);
        rc = sosx_block_strided_copy(ddev, dstr, stg, (ptrdiff_t)bsize, bsize, nblocks, ts, c.stream);
    } else if (sdev) {
        // pageable target: the kernel packs into the stage, a 2-D copy writes the blocks
        char *stg = (char *)stage(c, bbytes * nblocks);
        before_peer_read(c, read_pe, fn);
        rc = sosx_block_strided_copy(stg, (ptrdiff_t)bsize, sdev, sstr, bsize, nblocks, ts, c.stream);
        if (rc == SOSX_OK) {
            hip_check(release_system(c), fn);  // the copy engine reads HBM
            hip_check(hipMemcpy2DAsync(dst, (size_t)dstr * ts, stg, bbytes, bbytes, nblocks,
                                       hipMemcpyDeviceToHost, c.stream), fn);
        }
    } else {
        // both in pageable host memory of this process (pe == my_pe): the host moves the
        // blocks, after what the stream still has queued
        hip_check(sync_system(c), fn);
        for (size_t i = 0; i < nblocks; ++i)
            memcpy(dst + i * (size_t)dstr * ts, src + i * (size_t)sstr * ts, bbytes);
    }
    if (rc != SOSX_OK) raise_error("%s: block copy failed (%d)", fn, rc);
    hip_check(sync_system(c), fn);
}

void put_blocks(Ctx &c, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize, size_t nblocks,
                size_t ts, int pe, bool strided, const char *fn)
{
    const sos_rma_op op = {dest, source, tst, sst, bsize, nblocks, ts, pe, 1, strided};
    checked(op, fn);
    if (!bsize || !nblocks) return;
    blocks(c, translate(dest, pe), tst, (const char *)source, sst, bsize, nblocks, ts, st().my_pe, fn);
}

void get_blocks(Ctx &c, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize, size_t nblocks,
                size_t ts, int pe, bool strided, const char *fn)
{
    const sos_rma_op op = {source, dest, sst, tst, bsize, nblocks, ts, pe, 0, strided};
    checked(op, fn);
    if (!bsize || !nblocks) return;
    blocks(c, (char *)dest, tst, translate(source, pe), sst, bsize, nblocks, ts, pe, fn);
}

void put_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi, const char *fn)
{
    const sos_rma_op op = {dest, source, (ptrdiff_t)nelems, (ptrdiff_t)nelems, nelems, 1, type_size, pe, 1, 0};
    checked(op, fn);
    if (nelems) contiguous(c, translate(dest, pe), source, nelems * type_size, st().my_pe, nbi != 0, fn);
}

void get_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi, const char *fn)
{
    const sos_rma_op op = {source, dest, (ptrdiff_t)nelems, (ptrdiff_t)nelems, nelems, 1, type_size, pe, 0, 0};
    checked(op, fn);
    if (nelems) contiguous(c, dest, translate(source, pe), nelems * type_size, pe, nbi != 0, fn);
}

}  // namespace

// put on a context, for put-with-signal's composed form (signal.cpp)
void sosrt::rma_put_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                       const char *fn)
{
    put_on(c, dest, source, nelems, type_size, pe, nbi, fn);
}

// Every entry twice: on SHMEM_CTX_DEFAULT, and on the context the program names, whose
// `pe` is an index of its team (ctx_checked translates it before the checks).
extern "C" {

void sos_api_put(void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                 const char *fn)
{
    put_on(default_ctx(), dest, source, nelems, type_size, pe, nbi, fn);
}

void sos_api_get(void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                 const char *fn)
{
    get_on(default_ctx(), dest, source, nelems, type_size, pe, nbi, fn);
}

void sos_api_iput(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                  size_t type_size, int pe, const char *fn)
{
    put_blocks(default_ctx(), dest, source, tst, sst, 1, nelems, type_size, pe, true, fn);
}

void sos_api_iget(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                  size_t type_size, int pe, const char *fn)
{
    get_blocks(default_ctx(), dest, source, tst, sst, 1, nelems, type_size, pe, true, fn);
}

void sos_api_ibput(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                   size_t nblocks, size_t type_size, int pe, const char *fn)
{
    put_blocks(default_ctx(), dest, source, tst, sst, bsize, nblocks, type_size, pe, false, fn);
}

void sos_api_ibget(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                   size_t nblocks, size_t type_size, int pe, const char *fn)
{
    get_blocks(default_ctx(), dest, source, tst, sst, bsize, nblocks, type_size, pe, false, fn);
}

void sos_api_p(void *addr, const void *value, size_t type_size, int pe, const char *fn)
{
    sos_api_put(addr, value, 1, type_size, pe, 0, fn);
}

void sos_api_g(void *value, const void *addr, size_t type_size, int pe, const char *fn)
{
    sos_api_get(value, addr, 1, type_size, pe, 0, fn);
}

void sos_api_ctx_put(shmem_ctx_t ctx, void *dest, const void *source, size_t nelems, size_t type_size, int pe,
                     int nbi, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    put_on(c, dest, source, nelems, type_size, pe, nbi, fn);
}

void sos_api_ctx_get(shmem_ctx_t ctx, void *dest, const void *source, size_t nelems, size_t type_size, int pe,
                     int nbi, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    get_on(c, dest, source, nelems, type_size, pe, nbi, fn);
}

void sos_api_ctx_iput(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      size_t type_size, int pe, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    put_blocks(c, dest, source, tst, sst, 1, nelems, type_size, pe, true, fn);
}

void sos_api_ctx_iget(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      size_t type_size, int pe, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    get_blocks(c, dest, source, tst, sst, 1, nelems, type_size, pe, true, fn);
}

void sos_api_ctx_ibput(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                       size_t nblocks, size_t type_size, int pe, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    put_blocks(c, dest, source, tst, sst, bsize, nblocks, type_size, pe, false, fn);
}

void sos_api_ctx_ibget(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                       size_t nblocks, size_t type_size, int pe, const char *fn)
{
    Ctx &c = ctx_checked(ctx, &pe, fn);
    get_blocks(c, dest, source, tst, sst, bsize, nblocks, type_size, pe, false, fn);
}

void sos_api_ctx_p(shmem_ctx_t ctx, void *addr, const void *value, size_t type_size, int pe, const char *fn)
{
    sos_api_ctx_put(ctx, addr, value, 1, type_size, pe, 0, fn);
}

void sos_api_ctx_g(shmem_ctx_t ctx, void *value, const void *addr, size_t type_size, int pe, const char *fn)
{
    sos_api_ctx_get(ctx, value, addr, 1, type_size, pe, 0, fn);
}

void *sos_api_ptr(const void *dest, int pe)
{
    State &s = st();
    if (!s.initialized || s.finalized || pe < 0 || pe >= s.n_pes || !dest) return nullptr;
    if (pe == s.my_pe) return (void *)dest;
    if (!s.dev_heap.contains(dest, 1) || !heap_mapped(s)) return nullptr;
    return translate(dest, pe);
}

void *pshmem_ptr(const void *dest, int pe) { return sos_api_ptr(dest, pe); }
void *shmem_ptr(const void *dest, int pe) __attribute__((weak, alias("pshmem_ptr")));

}  // extern "C"
