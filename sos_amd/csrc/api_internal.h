// api_internal.h -- the generic entry points behind the typed reductions, team
// broadcasts and scans (reductions_gen.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "shmem.h"

#ifdef __cplusplus
#include <vector>

extern "C" {
#endif

// SHMEM_DEF_TO_ALL (src/collectives_c.c4:221-246)
void sos_api_to_all(void *target, const void *source, int nreduce, size_t type_size,
                    int PE_start, int logPE_stride, int PE_size, void *pWrk, long *pSync, int op,
                    int datatype, const char *fn);

// SHMEM_DEF_REDUCE (src/collectives_c.c4:248-269)
int sos_api_reduce(shmem_team_t team, void *dest, const void *source, size_t nreduce,
                   size_t type_size, int op, int datatype, const char *fn);

// SHMEM_DEF_BCAST (src/collectives_c.c4:402-429): team broadcast, root copies too
int sos_api_broadcast(shmem_team_t team, void *dest, const void *source, size_t nelems,
                      size_t type_size, int PE_root, const char *fn);

// SHMEM_DEF_INSCAN / SHMEM_DEF_EXSCAN (src/collectives_c.c4:294-340)
int sos_api_scan(shmem_team_t team, void *dest, const void *source, size_t nelems,
                 size_t type_size, int op, int datatype, int exclusive, const char *fn);

// SHMEM_DEF_FCOLLECT / SHMEM_DEF_ALLTOALL / SHMEM_DEF_ALLTOALLS
// (src/collectives_c.c4:536-556, :609-629, :687-705)
int sos_api_fcollect(shmem_team_t team, void *dest, const void *source, size_t nelems,
                     size_t type_size, const char *fn);
// SHMEM_DEF_COLLECT and shmem_collect32/64 (src/collectives_c.c4:432-503)
int sos_api_collect(shmem_team_t team, void *dest, const void *source, size_t nelems,
                    size_t type_size, const char *fn);
void sos_api_collect_active(void *target, const void *source, size_t nlong, size_t type_size,
                            int PE_start, int logPE_stride, int PE_size, long *pSync, const char *fn);
int sos_api_alltoall(shmem_team_t team, void *dest, const void *source, size_t nelems,
                     size_t type_size, const char *fn);
int sos_api_alltoalls(shmem_team_t team, void *dest, const void *source, ptrdiff_t dst,
                      ptrdiff_t sst, size_t nelems, size_t type_size, const char *fn);

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

// The argument checks of the entries above as one function of plain data, so that every
// refusal can be exercised without a running job: 0, or a code with its message.
enum {
    SOS_RMA_OK = 0,
    SOS_RMA_NOT_INITIALIZED = 1,
    SOS_RMA_BAD_PE = 2,
    SOS_RMA_NOT_POSITIVE = 3,    // iput / iget stride <= 0 (SHMEM_ERR_CHECK_POSITIVE)
    SOS_RMA_NOT_SYMMETRIC = 4,   // remote side outside every symmetric region, or past its end
    SOS_RMA_NULL_LOCAL = 5,
    SOS_RMA_STRIDE_LT_BSIZE = 6,
    SOS_RMA_OVERLAP = 7,         // pe == my_pe and the two extents intersect
    SOS_RMA_PEER_NOT_DEVICE_HEAP = 8,  // another PE's host heap, data segment or plain allocation
    SOS_RMA_NO_PATH = 9,         // another PE whose device heap is not mapped here
    SOS_RMA_BAD_TYPE_SIZE = 10,
};
enum { SOS_RMA_REGION_HOST_HEAP = 0, SOS_RMA_REGION_DEVICE_HEAP = 1, SOS_RMA_REGION_DATA = 2,
       SOS_RMA_REGION_DEVICE_ALLOC = 3 };
typedef struct {
    uintptr_t base;
    size_t size;
    int kind;
} sos_rma_region;
typedef struct {
    int initialized, my_pe, n_pes;
    int mapped;  // every peer's device heap is mapped on this PE
    int nregions;
    const sos_rma_region *regions;
} sos_rma_layout;
typedef struct {
    const void *remote, *local;
    ptrdiff_t remote_stride, local_stride;  // elements
    size_t bsize, nblocks, type_size;
    int pe;
    int put;      // the remote side is the target
    int strided;  // iput / iget: the strides must be positive
} sos_rma_op;
int sos_rma_check(const sos_rma_layout *layout, const sos_rma_op *op, char *msg, size_t msg_len);

// ---- atomic memory operations (amo.cpp) --------------------------------------------------
// SHMEM_DEF_SWAP ... SHMEM_DEF_FETCH_XOR and the nbi forms (src/atomic_c.c4:226-560,
// src/atomic_nbi_c.c4): op is a SOSX_AMO_*; value / cond point at the operands (NULL where
// the form has none); want_old: the old value goes to *fetch_out -- for the blocking forms
// the caller's local, filled when the call returns; for the nbi forms the program's
// `fetch`, filled no later than the next shmem_quiet.
void sos_api_amo(int op, void *target, const void *value, const void *cond, void *fetch_out, int want_old,
                 size_t type_size, int is_float, int pe, int nbi, const char *fn);
// Its checks in SOS's order -- initialized, PE, symmetric over type_size bytes -- then this
// library's own, over the layout struct of sos_rma_check: 0, or a SOS_RMA_* code (and
// SOS_AMO_NULL_FETCH) with its message.
enum { SOS_AMO_NULL_FETCH = 11 };  // an nbi fetching form without a place for the old value
typedef struct {
    const void *target;
    const void *fetch;  // looked at for the nbi forms only
    size_t type_size;
    int pe;
    int nbi;
} sos_amo_op;
int sos_amo_check(const sos_rma_layout *layout, const sos_amo_op *op, char *msg, size_t msg_len);

// ---- put with signal, signal operations, point-to-point waits (signal.cpp) ---------------
// SHMEM_DEF_PUT_SIGNAL / _NBI and the sized and mem forms (src/data_c.c4:684-784)
void sos_api_put_signal(void *dest, const void *source, size_t nelems, size_t type_size, uint64_t *sig_addr,
                        uint64_t signal, int sig_op, int pe, int nbi, const char *fn);
// shmemx_signal_set / shmemx_signal_add: sig_op on a peer's (or the caller's) signal word
void sos_api_signal_op(uint64_t *sig_addr, uint64_t signal, int sig_op, int pe, const char *fn);
// shmem_signal_fetch: the calling PE's own word
uint64_t sos_api_signal_fetch(const uint64_t *sig_addr, const char *fn);
// The kinds of a wait or test: one ivar, or the _all / _any / _some forms over nelems.
enum { SOS_SYNC_ONE = 0, SOS_SYNC_ALL = 1, SOS_SYNC_ANY = 2, SOS_SYNC_SOME = 3 };
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

// Their checks as plain functions over the layout struct of sos_rma_check: 0, or a code
// with a message that names the argument.  SOS's refusals in SOS's order, then this
// library's own.
enum { SOS_SIG_BAD_OP = 12,    // sig_op is neither SHMEM_SIGNAL_SET nor SHMEM_SIGNAL_ADD
       SOS_SYNC_BAD_CMP = 13 };  // the comparison is none of SHMEM_CMP_*
typedef struct {
    const void *target, *source, *sig_addr;
    size_t nelems, type_size;
    int sig_op;
    int pe;
} sos_put_signal_op;
int sos_put_signal_check(const sos_rma_layout *layout, const sos_put_signal_op *op, char *msg, size_t msg_len);
typedef struct {
    const void *ivars;
    size_t nelems, type_size;  // ONE: nelems is 1
    const void *status;        // const int[nelems] or NULL (ALL / ANY / SOME)
    const void *indices;       // size_t[nelems] (SOME)
    int kind;                  // SOS_SYNC_*
    int cmp;
} sos_sync_op;
int sos_sync_check(const sos_rma_layout *layout, const sos_sync_op *op, char *msg, size_t msg_len);

// The comparison of a wait or test over a snapshot of the ivars, as SOS's macros make it
// (SHMEM_TEST and the loops of src/synchronization_c.c4): `snapshot` holds nelems words of
// `width` (2, 4 or 8) bytes, compared signed or unsigned at that width against *value (or
// value[i], vector) for every i with status NULL or status[i] == 0.
//   ONE / ALL: returns 1 when (every unmasked) comparison holds;
//   ANY: returns 1 and *index = the lowest satisfied unmasked index, else *index = SIZE_MAX;
//   SOME: *count = how many hold, their indices ascending in `indices`; returns count > 0.
// nelems == 0 or everything masked: returns 1 (a wait returns at once) with
// *index = SIZE_MAX and *count = 0.  -1 for an argument it cannot use.
int sos_sync_eval(const void *snapshot, size_t nelems, size_t width, int is_signed, const int *status, int cmp,
                  const void *value, int vector, int kind, size_t *index, size_t *indices, size_t *count);

// ---- distributed locks (lock.cpp) --------------------------------------------------------
// shmem_set_lock / shmem_clear_lock / shmem_test_lock (src/lock_c.c:44-65)
void sos_api_set_lock(long *lock, const char *fn);
void sos_api_clear_lock(long *lock, const char *fn);
int sos_api_test_lock(long *lock, const char *fn);
// Their check over the layout struct of sos_rma_check, the same on every PE: SOS's
// (initialized, `lock` symmetric over sizeof(long)), then this library's own -- 8-byte
// alignment; with more than one PE the lock must be in the device symmetric heap
// (SOS_RMA_PEER_NOT_DEVICE_HEAP) and the heap mapped (SOS_RMA_NO_PATH).
typedef struct {
    const void *lock;
} sos_lock_op;
int sos_lock_check(const sos_rma_layout *layout, const sos_lock_op *op, char *msg, size_t msg_len);
// The messages of a wait that ran out and of a lock word that holds no PE id + 1, as plain
// functions.  awaited: 0 = SIGNAL (set_lock), 1 = NEXT (clear_lock).
enum { SOS_LOCK_AWAIT_SIGNAL = 0, SOS_LOCK_AWAIT_NEXT = 1 };
void sos_lock_expiry_message(const char *fn, const void *lock, int awaited, uint32_t data, double seconds, char *msg,
                             size_t msg_len);
void sos_lock_corrupt_message(const void *lock, int value, int n_pes, char *msg, size_t msg_len);

// ---- communication contexts (ctx.cpp; the checks: ctx_checks.cpp) ------------------------
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

// The handle check, the option check, the team-index translation and the stream-pool
// assignment as plain functions of data (ctx_checks.cpp has no HIP include): 0, or a code
// with its message.  A handle is looked up in the table of live contexts, never
// dereferenced: SHMEM_CTX_INVALID, a destroyed context and any other pointer are refused.
enum { SOS_CTX_OK = 0,
       SOS_CTX_BAD_PE = SOS_RMA_BAD_PE,  // the index is outside the context's team
       SOS_CTX_INVALID = 14,       // SHMEM_CTX_INVALID
       SOS_CTX_DESTROYED = 15,     // a handle shmem_ctx_destroy (or a team's / the library's teardown) freed
       SOS_CTX_UNKNOWN = 16,       // no context this library created
       SOS_CTX_BAD_OPTIONS = 17 }; // bits outside SHMEM_CTX_PRIVATE | _SERIALIZED | _NOSTORE
typedef struct {
    const void *handle;
    int start, stride, size;  // the context's team in world PEs
} sos_ctx_entry;
typedef struct {
    int nlive;
    const sos_ctx_entry *live;  // SHMEM_CTX_DEFAULT's entry included
    int ndead;
    const void *const *dead;    // handles destroyed and not reused since
} sos_ctx_table;
// *index: the entry of `handle` in live; *pe (or NULL: a call without one) goes from a team
// index to a world PE, refused with put / get's bad-PE message outside [0, size).
int sos_ctx_check(const sos_ctx_table *table, const void *handle, int *pe, int *index, char *msg, size_t msg_len);
int sos_ctx_options_check(long options, char *msg, size_t msg_len);
// SHMEMX_CTX_STREAMS as the environment gives it (NULL: unset): 1..31, default 3; -1 with a
// message for anything else.
int sos_ctx_pool_size(const char *env_value, char *msg, size_t msg_len);
// The pool slot of the context created after `created` others: round-robin.
int sos_ctx_stream_slot(unsigned long created, int pool_size);

#ifdef __cplusplus
}

// What rma.cpp and amo.cpp share.
namespace sosrt {
struct RmaLayout {
    std::vector<sos_rma_region> regions;
    sos_rma_layout l;
};
// the symmetric regions and the job's shape as they are now: the checks' input
void rma_layout_now(RmaLayout &out);
const sos_rma_region *rma_find_region(const sos_rma_layout *l, uintptr_t p);
const char *rma_region_name(int kind);
// the remote side's address on this PE
char *translate(const void *remote, int pe);
struct Ctx;
// Before a launch or copy on context `c` that reads peer `pe`'s heap: the acquire a wait
// since the context's last one left owed, on its stream, and the read counted.
void before_peer_read(Ctx &c, int pe, const char *fn);
// The entries behind sos_api_put / sos_api_amo and their ctx twins, for callers that
// already hold the context and a world PE (put-with-signal's composed form, the signal ops).
void rma_put_on(Ctx &c, void *dest, const void *source, size_t nelems, size_t type_size, int pe, int nbi,
                const char *fn);
void amo_on(Ctx &c, int op, void *target, const void *value, const void *cond, void *fetch_out, int want_old,
            size_t type_size, int is_float, int pe, int nbi, const char *fn);
// The address at which a kernel on this PE's GPU reaches the `bytes` bytes at p, or null
// where it cannot (rma.cpp).
char *device_view(const void *p, size_t bytes);
}  // namespace sosrt
#endif
