/*
 * ticket_counter.c -- a shared ticket counter with atomic memory operations on the device heap.
 *
 * PE 0 owns a counter and a table of P * K slots in device symmetric memory, all zero.
 * Every PE draws K tickets from the counter with shmem_long_atomic_fetch_add(&counter, 1, 0)
 * -- each call returns a ticket no other call returns -- and marks each ticket it drew with
 * shmem_int_atomic_inc(&table[ticket], 0).  The marks only enqueue; shmem_barrier_all
 * completes them.  PE 0 then copies the table to the host and checks that the counter is
 * P * K and every slot is exactly 1: no ticket was lost and none was drawn twice.
 * Prints "ticket_counter: OK (<n> PEs)" on PE 0 and exits 0, or reports the first bad slot.
 * With more than one PE the peers' heaps must be mapped: run under SHMEMX_TRANSPORT=p2p.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>

#define K 32 /* tickets per PE */

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    const size_t slots = (size_t) np * K;
    long *counter = shmemx_malloc_device(sizeof(long));
    int *table = shmemx_malloc_device(slots * sizeof(int));
    hipMemset(counter, 0, sizeof(long));
    hipMemset(table, 0, slots * sizeof(int));
    hipDeviceSynchronize();
    shmem_barrier_all(); /* PE 0's counter and table are zero before anyone draws */

    int bad = 0;
    for (int k = 0; k < K; ++k) {
        const long ticket = shmem_long_atomic_fetch_add(counter, 1, 0);
        if (ticket < 0 || (size_t) ticket >= slots) {
            fprintf(stderr, "ticket_counter: PE %d drew ticket %ld of %zu\n", me, ticket, slots);
            bad = 1;
            break;
        }
        shmem_int_atomic_inc(&table[ticket], 0);
    }
    shmem_barrier_all(); /* every mark is complete and visible on PE 0 */

    if (me == 0) {
        long drawn = -1;
        int *h = malloc(slots * sizeof(int));
        hipMemcpy(&drawn, counter, sizeof(long), hipMemcpyDeviceToHost);
        hipMemcpy(h, table, slots * sizeof(int), hipMemcpyDeviceToHost);
        if (drawn != (long) slots) {
            fprintf(stderr, "ticket_counter: the counter is %ld, expected %zu\n", drawn, slots);
            bad = 1;
        }
        for (size_t s = 0; s < slots && !bad; ++s)
            if (h[s] != 1) {
                fprintf(stderr, "ticket_counter: slot %zu was marked %d times\n", s, h[s]);
                bad = 1;
            }
        free(h);
    }
    /* every PE learns whether any PE saw a mismatch */
    int *in = shmem_malloc(sizeof(int)), *out = shmem_malloc(sizeof(int));
    *in = bad;
    shmem_int_max_reduce(SHMEM_TEAM_WORLD, out, in, 1);
    const int total = *out;
    shmem_free(out);
    shmem_free(in);
    shmemx_free_device(table);
    shmemx_free_device(counter);
    if (me == 0 && !total) printf("ticket_counter: OK (%d PEs)\n", np);
    shmem_finalize();
    return total != 0;
}
