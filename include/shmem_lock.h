/* shmem_lock.h -- SOS's distributed locks (mpp/shmem_c_func.h4:551-553): shmem_set_lock,
 * shmem_clear_lock, shmem_test_lock.  No contexts and no typed variants exist.
 *
 * `lock` is a symmetric `long`, zero on every PE before its first use and zero again after
 * the last shmem_clear_lock.  With more than one PE it must lie in the device symmetric
 * heap (shmemx_malloc_device), the only memory mapped across PEs; a single PE may lock any
 * symmetric word.  Included from shmem.h. */
#ifndef SHMEM_LOCK_H
#define SHMEM_LOCK_H

#ifdef __cplusplus
extern "C" {
#endif

SHMEM_FUNCTION_ATTRIBUTES void shmem_set_lock(long *lock);
SHMEM_FUNCTION_ATTRIBUTES void shmem_clear_lock(long *lock);
SHMEM_FUNCTION_ATTRIBUTES int shmem_test_lock(long *lock);

/* profiling interface: pshmem_* are the implementations, shmem_* weak aliases */
void pshmem_set_lock(long *lock);
void pshmem_clear_lock(long *lock);
int pshmem_test_lock(long *lock);

#ifdef __cplusplus
}
#endif

#endif /* SHMEM_LOCK_H */
