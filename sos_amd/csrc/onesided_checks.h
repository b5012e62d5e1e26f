// onesided_checks.h -- what the one-sided layer decides on plain data (onesided_checks.cpp):
// the argument checks of its five families, the comparison of a wait, and the texts a lock
// call can end the job with.  C linkage and plain C types: no HIP, no runtime state, so that
// every refusal can be exercised without a running job, from a program of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// ---- one-sided put / get ----------------------------------------------------------------
// The argument checks of sos_api_put ... sos_api_ibget as one function of plain data: 0, or
// a code with its message.
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

// ---- atomic memory operations ------------------------------------------------------------
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

// ---- put with signal, signal operations, point-to-point waits -----------------------------
// The kinds of a wait or test: one ivar, or the _all / _any / _some forms over nelems.
enum { SOS_SYNC_ONE = 0, SOS_SYNC_ALL = 1, SOS_SYNC_ANY = 2, SOS_SYNC_SOME = 3 };
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

// ---- distributed locks -------------------------------------------------------------------
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

// ---- communication contexts --------------------------------------------------------------
// The handle check, the option check, the team-index translation and the stream-pool
// assignment as plain functions of data: 0, or a code with its message.  A handle is looked up in the table of live contexts, never
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

namespace sosrt {  // the region of a layout that holds p, or null; a kind as the messages name it
const sos_rma_region *rma_find_region(const sos_rma_layout *l, uintptr_t p);
const char *rma_region_name(int kind);
}  // namespace sosrt
#endif
