/*
 * lock_counter.c -- a shared counter guarded by a distributed lock on the device heap.
 *
 * The lock and the counter are device symmetric memory, both zero; PE 0's copy of the counter
 * is the shared one.  Every PE does K rounds of shmem_set_lock, shmem_long_g the counter,
 * add one, shmem_long_p it back, shmem_clear_lock: a read-modify-write that is only correct
 * because the lock lets one PE at a time through and shmem_clear_lock completes the put
 * before the next PE can take the lock.  After a barrier PE 0 checks that the counter is
 * P * K and that the lock is zero again.  Prints "lock_counter: OK (<P> PEs, <K> rounds)" on
 * PE 0 and exits 0.
 *
 * A lock shared by several PEs must lie in the device symmetric heap (shmemx_malloc_device)
 * and be zeroed before its first use; the peers' heaps must be mapped: run under
 * SHMEMX_TRANSPORT=p2p.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>

#define K 20 /* rounds per PE */

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    long *lock = shmemx_malloc_device(sizeof(long));
    long *counter = shmemx_malloc_device(sizeof(long));
    hipMemset(lock, 0, sizeof(long));
    hipMemset(counter, 0, sizeof(long));
    hipDeviceSynchronize();
    shmem_barrier_all(); /* every PE's lock word is zero before anyone queues */

    for (int k = 0; k < K; ++k) {
        shmem_set_lock(lock);
        const long c = shmem_long_g(counter, 0);
        shmem_long_p(counter, c + 1, 0);
        shmem_clear_lock(lock);
    }
    shmem_barrier_all();

    int bad = 0;
    long mine = -1;
    hipMemcpy(&mine, lock, sizeof(long), hipMemcpyDeviceToHost);
    if (mine != 0) {
        fprintf(stderr, "lock_counter: PE %d's lock word is 0x%lx after the last clear_lock\n", me, mine);
        bad = 1;
    }
    if (me == 0) {
        long total = -1;
        hipMemcpy(&total, counter, sizeof(long), hipMemcpyDeviceToHost);
        if (total != (long) np * K) {
            fprintf(stderr, "lock_counter: the counter is %ld, expected %ld\n", total, (long) np * K);
            bad = 1;
        }
    }
    /* every PE learns whether any PE saw a mismatch */
    int *in = shmem_malloc(sizeof(int)), *out = shmem_malloc(sizeof(int));
    *in = bad;
    shmem_int_max_reduce(SHMEM_TEAM_WORLD, out, in, 1);
    const int any = *out;
    shmem_free(out);
    shmem_free(in);
    shmemx_free_device(counter);
    shmemx_free_device(lock);
    if (me == 0 && !any) printf("lock_counter: OK (%d PEs, %d rounds)\n", np, K);
    shmem_finalize();
    return any != 0;
}
