/*
 * collect_ragged.c -- shmem_collect on two or more PEs: PE i contributes i + 1 ints
 * (the values 100 * i + k, k = 0..i) and every PE receives the concatenation in PE
 * order, np * (np + 1) / 2 ints.  Runs on host symmetric-heap (shmem_malloc) and
 * device-heap (shmemx_malloc_device) buffers through the C11 generic shmem_collect, and
 * once with PE 0 contributing nothing (nelems == 0 is legal; the PE still takes part).
 * The ints of the target above the concatenation keep their value.
 * Prints "collect_ragged: OK (<P> PEs)" on PE 0 and exits 0, or reports the first mismatch.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define GUARD 4 /* ints above the result that must keep their value */

static void *sym_alloc(int device, size_t bytes)
{
    return device ? shmemx_malloc_device(bytes) : shmem_malloc(bytes);
}

static void sym_free(int device, void *p)
{
    if (device) shmemx_free_device(p);
    else shmem_free(p);
}

static void put(int device, void *sym, const void *host, size_t bytes)
{
    if (device) hipMemcpy(sym, host, bytes, hipMemcpyHostToDevice);
    else memcpy(sym, host, bytes);
}

static void get(int device, void *host, const void *sym, size_t bytes)
{
    if (device) hipMemcpy(host, sym, bytes, hipMemcpyDeviceToHost);
    else memcpy(host, sym, bytes);
}

/* PE p's contribution: p + 1 ints, or none from PE 0 when skip0 */
static size_t count_of(int p, int skip0) { return skip0 && p == 0 ? 0 : (size_t) p + 1; }

static int run(int device, int skip0)
{
    const int me = shmem_my_pe(), np = shmem_n_pes();
    const size_t cap = (size_t) np * (np + 1) / 2 + GUARD, mine = count_of(me, skip0);
    int *src = sym_alloc(device, (size_t) np * sizeof(int));
    int *dst = sym_alloc(device, cap * sizeof(int));
    int *h = malloc(cap * sizeof(int));
    for (size_t k = 0; k < mine; ++k) h[k] = 100 * me + (int) k;
    put(device, src, h, mine * sizeof(int));
    for (size_t k = 0; k < cap; ++k) h[k] = -1;
    put(device, dst, h, cap * sizeof(int));
    shmem_barrier_all();
    shmem_collect(SHMEM_TEAM_WORLD, dst, src, mine);
    get(device, h, dst, cap * sizeof(int));
    int bad = 0;
    size_t at = 0;
    for (int p = 0; p < np && !bad; ++p)
        for (size_t k = 0; k < count_of(p, skip0); ++k, ++at)
            if (h[at] != 100 * p + (int) k) {
                bad = 1;
                break;
            }
    for (size_t k = 0; k < GUARD && !bad; ++k, ++at)
        if (h[at] != -1) bad = 1;
    if (bad)
        fprintf(stderr, "collect_ragged: MISMATCH (%s heap%s) at int %zu (PE %d)\n",
                device ? "device" : "host", skip0 ? ", PE 0 empty" : "", at, me);
    free(h);
    shmem_barrier_all();
    sym_free(device, dst);
    sym_free(device, src);
    return bad;
}

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    int bad = 0;
    for (int device = 0; device < 2; ++device)
        for (int skip0 = 0; skip0 < 2; ++skip0) bad |= run(device, skip0);
    /* every PE learns whether any PE saw a mismatch */
    int *in = shmem_malloc(sizeof(int)), *out = shmem_malloc(sizeof(int));
    *in = bad;
    shmem_int_max_reduce(SHMEM_TEAM_WORLD, out, in, 1);
    const int total = *out;
    shmem_free(out);
    shmem_free(in);
    if (me == 0 && !total) printf("collect_ragged: OK (%d PEs)\n", np);
    shmem_finalize();
    return total != 0;
}
