// onesided.h -- the generic entry points behind the typed one-sided calls (rma_gen.cpp,
// amo_gen.cpp, signal_gen.cpp, ctx_gen.cpp, lock.cpp), and the host plumbing their five
// families share (onesided.cpp).
#pragma once
#include "onesided_checks.h"
#include "shmem.h"

#ifdef __cplusplus
extern "C" {
#endif

// ---- one-sided put / get (rma.cpp) -------------------------------------------------------
// SHMEM_DEF_PUT / _PUT_NBI / _GET / _GET_NBI and their sized and mem forms
// (src/data_c.c4:327-473); nbi: only enqueued on the library stream
void sos_api_put(void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                 const char *fn);
void sos_api_get(void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                 const char *fn);
// SHMEM_DEF_IPUT / _IGET (src/data_c.c4:475-497, :560-640): strides in elements
void sos_api_iput(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                  size_t type_size, int pe, const char *fn);
void sos_api_iget(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                  size_t type_size, int pe, const char *fn);
// SHMEM_DEF_IBPUT / _IBGET (src/data_c.c4:499-524): nblocks blocks of bsize elements
void sos_api_ibput(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                   size_t nblocks, size_t type_size, int pe, const char *fn);
void sos_api_ibget(void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                   size_t nblocks, size_t type_size, int pe, const char *fn);
// SHMEM_DEF_P / SHMEM_DEF_G (src/data_c.c4:300-325): a put / get of one element
void sos_api_p(void *addr, const void *value, size_t type_size, int pe, const char *fn);
void sos_api_g(void *value, const void *addr, size_t type_size, int pe, const char *fn);
// shmem_ptr: the address itself for the calling PE, the mapped address of a device-heap
// address on a mapped peer, NULL otherwise (never aborts)
void *sos_api_ptr(const void *dest, int pe);

// ---- atomic memory operations (amo.cpp) --------------------------------------------------
// SHMEM_DEF_SWAP ... SHMEM_DEF_FETCH_XOR and the nbi forms (src/atomic_c.c4:226-560,
// src/atomic_nbi_c.c4): op is a SOSX_AMO_*; value / cond point at the operands (NULL where
// the form has none); want_old: the old value goes to *fetch_out -- for the blocking forms
// the caller's local, filled when the call returns; for the nbi forms the program's
// `fetch`, filled no later than the next shmem_quiet.
void sos_api_amo(int op, void *target, const void *value, const void *cond, void *fetch_out, int want_old,
                 size_t type_size, int is_float, int pe, int nbi, const char *fn);

// ---- put with signal, signal operations, point-to-point waits (signal.cpp) ---------------
// SHMEM_DEF_PUT_SIGNAL / _NBI and the sized and mem forms (src/data_c.c4:684-784)
void sos_api_put_signal(void *dest, const void *source, size_t nelems, size_t type_size, uint64_t *sig_addr,
                        uint64_t signal, int sig_op, int pe, int nbi, const char *fn);
// shmemx_signal_set / shmemx_signal_add: sig_op on a peer's (or the caller's) signal word
void sos_api_signal_op(uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, const char *fn);
// shmem_signal_fetch: the calling PE's own word
uint64_t sos_api_signal_fetch(const uint64_t *sig_addr, const char *fn);
// shmem_<T>_wait_until[_all|_any|_some][_vector] (src/synchronization_c.c4:203-481): returns
// when the comparison holds -- for ONE and ALL 0, for ANY the index (SIZE_MAX: nothing to
// wait for), for SOME the count with `indices` filled.  `value` points at one value, or at
// nelems of them (vector).  *satisfied (or NULL) receives the ivar's value that satisfied a
// ONE wait (shmem_signal_wait_until).  cmp < 0: the deprecated shmem_<T>_wait, "until the
// ivar differs from value" (SHMEM_CMP_NE without the comparison check).
size_t sos_api_wait(void *ivars, size_t nelems, size_t *indices, const int *status, int cmp, const void *value,
                    int vector, int kind, size_t type_size, int is_signed, uint64_t *satisfied, const char *fn);
// shmem_<T>_test[_all|_any|_some][_vector] (:484-735): ONE probe; ONE and ALL return 0 / 1.
size_t sos_api_test(void *ivars, size_t nelems, size_t *indices, const int *status, int cmp, const void *value,
                    int vector, int kind, size_t type_size, int is_signed, const char *fn);

// ---- distributed locks (lock.cpp) --------------------------------------------------------
// shmem_set_lock / shmem_clear_lock / shmem_test_lock (src/lock_c.c:44-65)
void sos_api_set_lock(long *lock, const char *fn);
void sos_api_clear_lock(long *lock, const char *fn);
int sos_api_test_lock(long *lock, const char *fn);

// ---- communication contexts (ctx.cpp) ----------------------------------------------------
// The public shmem_ctx_* names are ctx_gen.cpp's, in a library of their own
// (libsos_amd_ctx.so) over these entries: libsos_amd.so exports no shmem_ctx_ name.
// The ctx twin of every entry above that has one in SOS: the handle is checked, `pe` is
// read as an index of the context's team, and the operation runs on the context's stream.
int sos_api_ctx_create(long options, shmem_ctx_t *ctx);
int sos_api_team_create_ctx(shmem_team_t team, long options, shmem_ctx_t *ctx);
int sos_api_ctx_get_team(shmem_ctx_t ctx, shmem_team_t *team);
void sos_api_ctx_destroy(shmem_ctx_t ctx);
void sos_api_ctx_quiet(shmem_ctx_t ctx);
void sos_api_ctx_fence(shmem_ctx_t ctx);
void sos_api_ctx_put(shmem_ctx_t ctx, void *dest, const void *source, size_t nelems, size_t type_size, int pe,
                     int nbi, const char *fn);
void sos_api_ctx_get(shmem_ctx_t ctx, void *dest, const void *source, size_t nelems, size_t type_size, int pe,
                     int nbi, const char *fn);
void sos_api_ctx_iput(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      size_t type_size, int pe, const char *fn);
void sos_api_ctx_iget(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t nelems,
                      size_t type_size, int pe, const char *fn);
void sos_api_ctx_ibput(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                       size_t nblocks, size_t type_size, int pe, const char *fn);
void sos_api_ctx_ibget(shmem_ctx_t ctx, void *dest, const void *source, ptrdiff_t tst, ptrdiff_t sst, size_t bsize,
                       size_t nblocks, size_t type_size, int pe, const char *fn);
void sos_api_ctx_p(shmem_ctx_t ctx, void *addr, const void *value, size_t type_size, int pe, const char *fn);
void sos_api_ctx_g(shmem_ctx_t ctx, void *value, const void *addr, size_t type_size, int pe, const char *fn);
void sos_api_ctx_amo(shmem_ctx_t ctx, int op, void *target, const void *value, const void *cond, void *fetch_out,
                     int want_old, size_t type_size, int is_float, int pe, int nbi, const char *fn);
void sos_api_ctx_put_signal(shmem_ctx_t ctx, void *dest, const void *source, size_t nelems, size_t type_size,
                            uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, int nbi, const char *fn);
void sos_api_ctx_signal_op(shmem_ctx_t ctx, uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, const char *fn);

#ifdef __cplusplus
}

#include <vector>

typedef struct ihipStream_t *hipStream_t;  // as HIP has it: the generated bindings include this without HIP

namespace sosrt {  // the host plumbing the five families share (onesided.cpp)
struct Ctx;
struct State;
struct RmaLayout {
    std::vector<sos_rma_region> regions;
    sos_rma_layout l;
};
// the symmetric regions and the job's shape as they are now: the checks' input
void rma_layout_now(RmaLayout &out);
bool heap_mapped(const State &s);                            // every PE's device heap is mapped on this one
[[noreturn]] void refused(const char *fn, const char *msg);  // ends the job with "<fn>: <msg>"
// The remote side's address on this PE: a device-heap address belongs to PE `pe` at
// peer_heap[pe] + (addr - peer_heap[my_pe]) (every PE maps every heap under
// SHMEMX_TRANSPORT=p2p|both); pe == my_pe needs no mapping and may name any symmetric memory.
char *translate(const void *remote, int pe);
// The address at which a kernel on this PE's GPU reaches the `bytes` bytes at p, or null
// where it cannot (pageable host memory, or an extent only partly registered with HIP, such
// as a data segment whose first page was rounded off).  Device memory is its own address;
// host memory that HIP allocated or registered is reached through the device pointer HIP
// reports for it, which need not equal p.
char *device_view(const void *p, size_t bytes);
// Before a launch or copy on context `c` that reads peer `pe`'s heap: the acquire a wait
// since the context's last one left owed, on its stream, and the read counted.
void before_peer_read(Ctx &c, int pe, const char *fn);
// The consumer half after a wait for a peer returned (a barrier, a satisfied wait or test,
// an acquired lock): its bytes may have arrived, so the wait is noted and the acquire follows
// at once on `stream` -- only where peers can store here at all (several PEs, heaps mapped).
void after_peer_wait(hipStream_t stream, const char *fn);
// A pinned host buffer with its device view.  reserve: at least `bytes` -- the first call
// allocates; a larger request completes `stream` first (a kernel queued there may still
// write the old buffer), releases and allocates anew.  `tag` names the buffer in a HIP error.
struct Pinned {
    void *host = nullptr, *dev = nullptr;
    size_t bytes = 0;
    void reserve(size_t want, hipStream_t stream, const char *tag, const char *fn);
    void release();
};
// The entries behind sos_api_put / sos_api_amo and their ctx twins, for callers that
// already hold the context and a world PE (put-with-signal's composed form, the signal ops).
void rma_put_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                const char *fn);
void amo_on(Ctx &c, int op, void *target, const void *value, const void *cond, void *fetch_out, int want_old,
            size_t type_size, int is_float, int pe, int nbi, const char *fn);

#pragma GCC visibility push(hidden)
// The layout as it is now, `check` over it and `op`, and what it refuses raised in fn's name.
template <class Op>
void checked(int (*check)(const sos_rma_layout *, const Op *, char *, size_t), const Op &op, const char *fn)
{
    RmaLayout lay;
    rma_layout_now(lay);
    char msg[512];
    if (check(&lay.l, &op, msg, sizeof(msg)) != SOS_RMA_OK) refused(fn, msg);
}
#pragma GCC visibility pop
}  // namespace sosrt
#endif
