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

#ifdef __cplusplus
}
#endif

#include "onesided.h"  // the one-sided entries, their checks and the plumbing they share
