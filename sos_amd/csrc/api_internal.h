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
// Before a launch or copy that reads peer `pe`'s heap: the acquire a wait since the last
// one left owed, and the read counted.
void before_peer_read(int pe, const char *fn);
// The address at which a kernel on this PE's GPU reaches the `bytes` bytes at p, or null
// where it cannot (rma.cpp).
char *device_view(const void *p, size_t bytes);
}  // namespace sosrt
#endif
