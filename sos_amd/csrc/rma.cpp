// rma.cpp -- one-sided put / get on the device symmetric heap: the generic entries behind
// shmem_put / get / p / g / iput / iget, shmemx_ibput / ibget and shmem_ptr (rma_gen.cpp).
//
// SOS's checks in SOS's order (src/data_c.c4:300-680) are one function of plain data
// (sos_rma_check, onesided_checks.cpp); the entries raise what it refuses (checked),
// translate the remote address (translate, onesided.cpp) and move the bytes on the library
// stream:
//
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
//    issued after the last wait for a peer (before_peer_read, onesided.cpp);
//  * contexts: "the library stream" above is the stream of the context the call names --
//    SHMEM_CTX_DEFAULT for the plain forms -- with that context's release event, stage and
//    acquire flag (ctx.cpp).
#include <hip/hip_runtime.h>
#include <string.h>

#include "onesided.h"
#include "runtime.h"
#include "shmemx.h"
#include "sosx.h"

using namespace sosrt;

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
    checked(sos_rma_check, op, fn);
    if (!bsize || !nblocks) return;
    blocks(c, translate(dest, pe), tst, (const char *)source, sst, bsize, nblocks, ts, st().my_pe, fn);
}

void get_blocks(Ctx &c, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize, size_t nblocks,
                size_t ts, int pe, bool strided, const char *fn)
{
    const sos_rma_op op = {source, dest, sst, tst, bsize, nblocks, ts, pe, 0, strided};
    checked(sos_rma_check, op, fn);
    if (!bsize || !nblocks) return;
    blocks(c, (char *)dest, tst, translate(source, pe), sst, bsize, nblocks, ts, pe, fn);
}

void get_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi, const char *fn)
{
    const sos_rma_op op = {source, dest, (ptrdiff_t)nelems, (ptrdiff_t)nelems, nelems, 1, type_size, pe, 0, 0};
    checked(sos_rma_check, op, fn);
    if (nelems) contiguous(c, dest, translate(source, pe), nelems * type_size, pe, nbi != 0, fn);
}

}  // namespace

// put on a context: the entries below, and put-with-signal's composed form (signal.cpp)
void sosrt::rma_put_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                       const char *fn)
{
    const sos_rma_op op = {dest, source, (ptrdiff_t)nelems, (ptrdiff_t)nelems, nelems, 1, type_size, pe, 1, 0};
    checked(sos_rma_check, op, fn);
    if (nelems) contiguous(c, translate(dest, pe), source, nelems * type_size, st().my_pe, nbi != 0, fn);
}

// Every entry twice: on SHMEM_CTX_DEFAULT, and on the context the program names, whose
// `pe` is an index of its team (ctx_checked translates it before the checks).
extern "C" {

void sos_api_put(void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                 const char *fn)
{
    rma_put_on(default_ctx(), dest, source, nelems, type_size, pe, nbi, fn);
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
    rma_put_on(c, dest, source, nelems, type_size, pe, nbi, fn);
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
