/*
 * halo_signal.c -- a ring halo exchange with put-with-signal: no barrier per message.
 *
 * Every PE owns N interior cells in device symmetric memory, with one halo cell on each
 * side.  In each of STEPS steps a PE sends its first cell to its left neighbour's right
 * halo and its last cell to its right neighbour's left halo with shmem_putmem_signal_nbi,
 * adding 1 to the neighbour's signal word for that side; it then waits for its own two
 * signals -- the left one alone with shmem_signal_wait_until, then both at once with
 * shmem_uint64_wait_until_all -- and only then reads its halos.  The value a cell carries
 * encodes (owner, step), so a halo read before its put arrived, or a put that overtook its
 * signal, is caught.  A neighbour may run one step ahead, never two: it cannot finish step
 * s + 1 without this PE's step s + 1 halo, so each side has two halo slots used in turn.
 * Prints "halo_signal: OK (<n> PEs, <steps> steps)" on PE 0 and exits 0.
 * With more than one PE the peers' heaps must be mapped: run under SHMEMX_TRANSPORT=p2p.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>

#define N 1024
#define STEPS 20

static long cell(int owner, int step, int i) { return 1000000L * owner + 1000L * step + i; }

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    const int left = (me + np - 1) % np, right = (me + 1) % np;
    long *interior = shmemx_malloc_device(N * sizeof(long));
    long *halo = shmemx_malloc_device(4 * sizeof(long));       /* [slot][0 = left side, 1 = right side] */
    uint64_t *sig = shmemx_malloc_device(2 * sizeof(uint64_t)); /* arrivals from the left, from the right */
    long *h = malloc(N * sizeof(long));
    hipMemset(halo, 0, 4 * sizeof(long));
    hipMemset(sig, 0, 2 * sizeof(uint64_t));
    hipDeviceSynchronize();
    shmem_barrier_all(); /* every PE's signals are zero before anyone adds to them */

    int bad = 0;
    for (int s = 1; s <= STEPS && !bad; ++s) {
        const int slot = s % 2;
        for (int i = 0; i < N; ++i) h[i] = cell(me, s, i);
        hipMemcpy(interior, h, N * sizeof(long), hipMemcpyHostToDevice);
        /* my first cell is my left neighbour's right halo, my last cell my right neighbour's left halo */
        shmem_putmem_signal_nbi(&halo[2 * slot + 1], &interior[0], sizeof(long), &sig[1], 1, SHMEM_SIGNAL_ADD, left);
        shmem_putmem_signal_nbi(&halo[2 * slot + 0], &interior[N - 1], sizeof(long), &sig[0], 1, SHMEM_SIGNAL_ADD, right);
        const uint64_t seen = shmem_signal_wait_until(&sig[0], SHMEM_CMP_GE, (uint64_t) s);
        shmem_uint64_wait_until_all(sig, 2, NULL, SHMEM_CMP_GE, (uint64_t) s);
        long got[2];
        hipMemcpy(got, &halo[2 * slot], sizeof(got), hipMemcpyDeviceToHost);
        if (seen < (uint64_t) s || got[0] != cell(left, s, N - 1) || got[1] != cell(right, s, 0)) {
            fprintf(stderr, "halo_signal: PE %d step %d: signal %llu, halos %ld %ld, expected %ld %ld\n", me, s,
                    (unsigned long long) seen, got[0], got[1], cell(left, s, N - 1), cell(right, s, 0));
            bad = 1;
        }
    }
    shmem_barrier_all();
    if (shmem_signal_fetch(&sig[0]) != STEPS || shmem_signal_fetch(&sig[1]) != STEPS) {
        fprintf(stderr, "halo_signal: PE %d: final signals are not %d\n", me, STEPS);
        bad = 1;
    }
    int *flag = shmem_malloc(sizeof(int)), *any = shmem_malloc(sizeof(int));
    *flag = bad;
    shmem_int_max_reduce(SHMEM_TEAM_WORLD, any, flag, 1);
    if (me == 0 && !*any) printf("halo_signal: OK (%d PEs, %d steps)\n", np, STEPS);
    const int rc = *any;
    shmem_free(any);
    shmem_free(flag);
    free(h);
    shmemx_free_device(sig);
    shmemx_free_device(halo);
    shmemx_free_device(interior);
    shmem_finalize();
    return rc;
}
