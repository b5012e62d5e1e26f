/*
 * halo_put.c -- a one-sided halo exchange with shmemx_ibput on the device heap.
 *
 * Every PE owns a ROWS x (COLS + HALO) tile of floats in device symmetric memory: COLS
 * interior columns and, left of them, HALO halo columns.  Cell (r, c) of PE p's interior
 * holds 1000 * p + 10 * r + c.  Each PE puts its LAST HALO interior columns -- one block of
 * HALO floats per row, a row apart -- into the halo columns of its right neighbour with one
 * shmemx_float_ibput, calls shmem_barrier_all, copies its tile to the host and checks that
 * the halo holds the left neighbour's columns and that its own interior is untouched.
 * Prints "halo_put: OK (<n> PEs)" on PE 0 and exits 0, or reports the first mismatch.
 * Needs two or more PEs (on one PE the source and target would overlap, which put
 * refuses) with the peers' heaps mapped: run under SHMEMX_TRANSPORT=p2p.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>

#define ROWS 37
#define COLS 50
#define HALO 3
#define PITCH (COLS + HALO)

static float cell(int pe, int r, int c) { return (float) (1000 * pe + 10 * r + c); }

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    const int right = (me + 1) % np, left = (me + np - 1) % np;
    const size_t cells = (size_t) ROWS * PITCH;
    float *tile = shmemx_malloc_device(cells * sizeof(float));
    float *h = malloc(cells * sizeof(float));
    for (int r = 0; r < ROWS; ++r) {
        for (int c = 0; c < HALO; ++c) h[r * PITCH + c] = -1.0f;
        for (int c = 0; c < COLS; ++c) h[r * PITCH + HALO + c] = cell(me, r, c);
    }
    hipMemcpy(tile, h, cells * sizeof(float), hipMemcpyHostToDevice);
    shmem_barrier_all(); /* every tile is filled before anyone puts into it */

    /* my last HALO interior columns -> the right neighbour's halo columns */
    shmemx_ibput(tile, tile + HALO + COLS - HALO, PITCH, PITCH, HALO, ROWS, right);
    shmem_barrier_all(); /* the puts are complete and visible on every PE */

    hipMemcpy(h, tile, cells * sizeof(float), hipMemcpyDeviceToHost);
    int bad = 0;
    for (int r = 0; r < ROWS && !bad; ++r) {
        for (int c = 0; c < HALO && !bad; ++c)
            if (h[r * PITCH + c] != cell(left, r, COLS - HALO + c)) {
                fprintf(stderr, "halo_put: PE %d halo (%d, %d) = %g, expected %g\n", me, r, c,
                        h[r * PITCH + c], cell(left, r, COLS - HALO + c));
                bad = 1;
            }
        for (int c = 0; c < COLS && !bad; ++c)
            if (h[r * PITCH + HALO + c] != cell(me, r, c)) {
                fprintf(stderr, "halo_put: PE %d interior (%d, %d) was overwritten\n", me, r, c);
                bad = 1;
            }
    }
    free(h);
    /* every PE learns whether any PE saw a mismatch */
    int *in = shmem_malloc(sizeof(int)), *out = shmem_malloc(sizeof(int));
    *in = bad;
    shmem_int_max_reduce(SHMEM_TEAM_WORLD, out, in, 1);
    const int total = *out;
    shmem_free(out);
    shmem_free(in);
    shmemx_free_device(tile);
    if (me == 0 && !total) printf("halo_put: OK (%d PEs)\n", np);
    shmem_finalize();
    return total != 0;
}
