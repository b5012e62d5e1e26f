/*
 * alltoall_types.c -- end-to-end check of fcollect, alltoall and alltoalls on two or
 * more PEs, on host symmetric-heap (shmem_malloc) and device-heap (shmemx_malloc_device)
 * buffers, against closed forms:
 *   - a P x P block matrix of long transposed with the C11 generic shmem_alltoall;
 *   - an int gather with shmem_int_fcollect;
 *   - shmem_double_alltoalls with dst = 2, sst = 3 (gaps of the target keep their value).
 * Prints "alltoall_types: OK (<P> PEs)" on PE 0 and exits 0, or reports the first mismatch.
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NB 1001 /* elements per block */
#define DST 2
#define SST 3

static int fail(const char *what, int device, size_t i)
{
    fprintf(stderr, "alltoall_types: MISMATCH in %s (%s heap) at %zu (PE %d)\n", what,
            device ? "device" : "host", i, shmem_my_pe());
    return 1;
}

static void *sym_alloc(int device, size_t bytes)
{
    return device ? shmemx_malloc_device(bytes) : shmem_malloc(bytes);
}

static void sym_free(int device, void *p)
{
    if (device) shmemx_free_device(p);
    else shmem_free(p);
}

/* host <-> symmetric buffer of either residency */
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

/* element k of block j of PE p's alltoall source */
static long cell(int p, int j, size_t k) { return 1000000L * p + 1000L * j + (long) (k % 997); }

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    const size_t N = (size_t) np * NB;
    int bad = 0;

    for (int device = 0; device <= 1; device++) {  /* every PE makes every call, failed or not */
        /* transpose: block j of my source becomes block `me` of PE j's target */
        long *hl = malloc(N * sizeof(long));
        long *ls = sym_alloc(device, N * sizeof(long)), *ld = sym_alloc(device, N * sizeof(long));
        for (int j = 0; j < np; j++)
            for (size_t k = 0; k < NB; k++) hl[(size_t) j * NB + k] = cell(me, j, k);
        put(device, ls, hl, N * sizeof(long));
        shmem_alltoall(SHMEM_TEAM_WORLD, ld, ls, NB);
        get(device, hl, ld, N * sizeof(long));
        for (int j = 0; j < np && !bad; j++)
            for (size_t k = 0; k < NB && !bad; k++)
                if (hl[(size_t) j * NB + k] != cell(j, me, k)) bad = fail("shmem_alltoall(long)", device, (size_t) j * NB + k);
        sym_free(device, ld);
        sym_free(device, ls);
        free(hl);

        /* gather: every PE ends with every PE's NB ints, in PE order */
        int *hi = malloc(N * sizeof(int));
        int *is = sym_alloc(device, NB * sizeof(int)), *id = sym_alloc(device, N * sizeof(int));
        for (size_t k = 0; k < NB; k++) hi[k] = 7919 * me + (int) k;
        put(device, is, hi, NB * sizeof(int));
        shmem_int_fcollect(SHMEM_TEAM_WORLD, id, is, NB);
        get(device, hi, id, N * sizeof(int));
        for (int p = 0; p < np && !bad; p++)
            for (size_t k = 0; k < NB && !bad; k++)
                if (hi[(size_t) p * NB + k] != 7919 * p + (int) k) bad = fail("shmem_int_fcollect", device, (size_t) p * NB + k);
        sym_free(device, id);
        sym_free(device, is);
        free(hi);

        /* strided: element k of the packed operand sits SST apart in the source and DST
           apart in the target; the target's gaps keep -1 */
        const size_t sn = (N - 1) * SST + 1, dn = (N - 1) * DST + 1;
        double *hs = malloc(sn * sizeof(double)), *hd = malloc(dn * sizeof(double));
        double *ss = sym_alloc(device, sn * sizeof(double)), *sd = sym_alloc(device, dn * sizeof(double));
        for (size_t i = 0; i < sn; i++) hs[i] = -2.0;
        for (size_t i = 0; i < dn; i++) hd[i] = -1.0;
        for (int j = 0; j < np; j++)
            for (size_t k = 0; k < NB; k++) hs[((size_t) j * NB + k) * SST] = 0.5 * (double) cell(me, j, k);
        put(device, ss, hs, sn * sizeof(double));
        put(device, sd, hd, dn * sizeof(double));
        shmem_double_alltoalls(SHMEM_TEAM_WORLD, sd, ss, DST, SST, NB);
        get(device, hd, sd, dn * sizeof(double));
        for (size_t i = 0; i < dn && !bad; i++) {
            const size_t e = i / DST, j = e / NB, k = e % NB;
            const double want = i % DST ? -1.0 : 0.5 * (double) cell((int) j, me, k);
            if (hd[i] != want) bad = fail("shmem_double_alltoalls", device, i);
        }
        sym_free(device, sd);
        sym_free(device, ss);
        free(hd);
        free(hs);
    }

    shmem_barrier_all();
    if (me == 0 && !bad) printf("alltoall_types: OK (%d PEs)\n", np);
    shmem_finalize();
    return bad;
}
