/*
 * halo_ctx.c -- halo_put.c with the two directions of the exchange on two communication
 * contexts, each completed by its own shmem_ctx_quiet.
 *
 * Every PE owns a ROWS x (HALO + COLS + HALO) tile of floats in device symmetric memory: COLS
 * interior columns with HALO halo columns on either side.  Cell (r, c) of PE p's interior
 * holds 1000 * p + 10 * r + c.  Each PE puts its LAST HALO interior columns into the LEFT
 * halo of its right neighbour on context `east`, and its FIRST HALO interior columns into
 * the RIGHT halo of its left neighbour on context `west` -- one shmemx_ibput each, through
 * the generic with a leading context.  The two contexts sit on streams of their own, so
 * neither direction is ordered behind the other; shmem_ctx_quiet(east) completes the
 * eastward puts alone and shmem_ctx_quiet(west) the westward ones.  After a barrier every
 * PE copies its tile to the host and checks both halos and that its interior is untouched.
 * Prints "halo_ctx: OK (<n> PEs)" on PE 0 and exits 0, or reports the first mismatch.
 * Needs two or more PEs with the peers' heaps mapped: run under SHMEMX_TRANSPORT=p2p.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>

#define ROWS 37
#define COLS 50
#define HALO 3
#define PITCH (HALO + COLS + HALO)

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
        for (int c = 0; c < HALO; ++c) h[r * PITCH + c] = h[r * PITCH + HALO + COLS + c] = -1.0f;
        for (int c = 0; c < COLS; ++c) h[r * PITCH + HALO + c] = cell(me, r, c);
    }
    hipMemcpy(tile, h, cells * sizeof(float), hipMemcpyHostToDevice);
    shmem_ctx_t east, west;
    if (shmem_ctx_create(0, &east) || shmem_ctx_create(0, &west)) {
        fprintf(stderr, "halo_ctx: PE %d cannot create its contexts\n", me);
        shmem_global_exit(2);
    }
    shmem_barrier_all(); /* every tile is filled before anyone puts into it */

    /* my last HALO interior columns -> the right neighbour's left halo */
    shmemx_ibput(east, tile, tile + HALO + COLS - HALO, PITCH, PITCH, HALO, ROWS, right);
    /* my first HALO interior columns -> the left neighbour's right halo */
    shmemx_ibput(west, tile + HALO + COLS, tile + HALO, PITCH, PITCH, HALO, ROWS, left);
    shmem_ctx_quiet(east); /* the eastward puts are delivered */
    shmem_ctx_quiet(west); /* the westward ones */
    shmem_barrier_all();   /* every PE has done both */

    hipMemcpy(h, tile, cells * sizeof(float), hipMemcpyDeviceToHost);
    int bad = 0;
    for (int r = 0; r < ROWS && !bad; ++r) {
        for (int c = 0; c < HALO && !bad; ++c) {
            if (h[r * PITCH + c] != cell(left, r, COLS - HALO + c)) {
                fprintf(stderr, "halo_ctx: PE %d left halo (%d, %d) = %g, expected %g\n", me, r, c,
                        h[r * PITCH + c], cell(left, r, COLS - HALO + c));
                bad = 1;
            }
            if (h[r * PITCH + HALO + COLS + c] != cell(right, r, c)) {
                fprintf(stderr, "halo_ctx: PE %d right halo (%d, %d) = %g, expected %g\n", me, r, c,
                        h[r * PITCH + HALO + COLS + c], cell(right, r, c));
                bad = 1;
            }
        }
        for (int c = 0; c < COLS && !bad; ++c)
            if (h[r * PITCH + HALO + c] != cell(me, r, c)) {
                fprintf(stderr, "halo_ctx: PE %d interior (%d, %d) was overwritten\n", me, r, c);
                bad = 1;
            }
    }
    free(h);
    shmem_ctx_destroy(east);
    shmem_ctx_destroy(west);
    /* every PE learns whether any PE saw a mismatch */
    int *in = shmem_malloc(sizeof(int)), *out = shmem_malloc(sizeof(int));
    *in = bad;
    shmem_int_max_reduce(SHMEM_TEAM_WORLD, out, in, 1);
    const int total = *out;
    shmem_free(out);
    shmem_free(in);
    shmemx_free_device(tile);
    if (me == 0 && !total) printf("halo_ctx: OK (%d PEs)\n", np);
    shmem_finalize();
    return total != 0;
}
