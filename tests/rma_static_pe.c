/*
 * rma_static_pe.c -- the self-PE strided and block forms on STATIC data and on the host
 * symmetric heap (one process per PE, tools/oshrun; built by tests/test_gpu_rma_multipe.py).
 *
 * For pe == shmem_my_pe() the symmetric side of a put or get may be any symmetric memory.
 * Static data is kernel-reachable only where shmem_init registered the data segment with
 * HIP; under SHMEMX_REGISTER_DATA=0 it is pageable host memory and the library has to
 * stage it.  Each PE runs, with itself as the target PE,
 *   shmem_int_iput / iget, shmemx_int_ibput / ibget, shmem_int_put / get
 * with the symmetric side in .bss (and, for the same calls, in shmem_malloc memory) and the
 * local side in device memory, in malloc memory and in another static array, and checks
 * every int of the target on the host: the blocks moved, everything else kept its canary.
 * Prints "rma_static: PE <i>/<n> OK (<k> checks, data segment <registered|pageable>)".
 */
#include <shmem.h>
#include <shmemx.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define N 4096                /* ints per buffer */
#define CANARY 0x6B6B6B6B

static int sym_static[N];     /* the symmetric side */
static int loc_static[N];     /* a local side that is static too */

static int checks, bad;

static int value(int tag, int k) { return tag * 100000 + k; }

/* expected[k] after blocks of bsize at tst from src blocks at sst */
static void expect(int *exp, const int *src, long tst, long sst, size_t bsize, size_t nblocks)
{
    for (int k = 0; k < N; ++k) exp[k] = CANARY;
    for (size_t i = 0; i < nblocks; ++i)
        for (size_t j = 0; j < bsize; ++j) exp[i * tst + j] = src[i * sst + j];
}

static void compare(const int *exp, const int *got, const char *what, const char *where)
{
    ++checks;
    for (int k = 0; k < N; ++k)
        if (exp[k] != got[k]) {
            if (!bad++) fprintf(stderr, "rma_static: %s (%s): int %d is %d, expected %d\n", what, where, k, got[k], exp[k]);
            return;
        }
}

/* kind of the local side: 0 device memory, 1 malloc, 2 static */
static int *local_alloc(int kind, int **dev)
{
    *dev = NULL;
    if (kind == 0) {
        hipMalloc((void **) dev, N * sizeof(int));
        return *dev;
    }
    return kind == 1 ? malloc(N * sizeof(int)) : loc_static;
}

static void local_write(int kind, int *p, const int *h)
{
    if (kind == 0) hipMemcpy(p, h, N * sizeof(int), hipMemcpyHostToDevice);
    else memcpy(p, h, N * sizeof(int));
}

static void local_read(int kind, int *h, const int *p)
{
    if (kind == 0) hipMemcpy(h, p, N * sizeof(int), hipMemcpyDeviceToHost);
    else memcpy(h, p, N * sizeof(int));
}

static void local_free(int kind, int *p)
{
    if (kind == 0) hipFree(p);
    else if (kind == 1) free(p);
}

/* one shape, every direction, symmetric side `sym` (host memory of this process) */
static void run(int *sym, const char *where, int kind, long tst, long sst, size_t bsize, size_t nblocks)
{
    const int me = shmem_my_pe();
    static int h[N], exp[N], got[N];
    int *dev, *loc = local_alloc(kind, &dev);
    char what[128];
    /* put forms: local -> symmetric */
    for (int form = 0; form < 3; ++form) {
        if (form == 0 && bsize != 1) continue;          /* iput */
        if (form == 2 && (tst != (long) bsize || sst != (long) bsize)) continue; /* put: contiguous */
        for (int k = 0; k < N; ++k) h[k] = value(10 + form, k);
        local_write(kind, loc, h);
        for (int k = 0; k < N; ++k) sym[k] = CANARY;
        if (form == 0) shmem_int_iput(sym, loc, tst, sst, nblocks, me);
        else if (form == 1) shmemx_int_ibput(sym, loc, tst, sst, bsize, nblocks, me);
        else shmem_int_put(sym, loc, bsize * nblocks, me);
        expect(exp, h, tst, sst, bsize, nblocks);
        snprintf(what, sizeof(what), "%s local %d tst %ld sst %ld bsize %zu nblocks %zu",
                 form == 0 ? "iput" : form == 1 ? "ibput" : "put", kind, tst, sst, bsize, nblocks);
        compare(exp, sym, what, where);
    }
    /* get forms: symmetric -> local */
    for (int form = 0; form < 3; ++form) {
        if (form == 0 && bsize != 1) continue;
        if (form == 2 && (tst != (long) bsize || sst != (long) bsize)) continue;
        for (int k = 0; k < N; ++k) sym[k] = value(20 + form, k);
        for (int k = 0; k < N; ++k) h[k] = CANARY;
        local_write(kind, loc, h);
        if (form == 0) shmem_int_iget(loc, sym, tst, sst, nblocks, me);
        else if (form == 1) shmemx_int_ibget(loc, sym, tst, sst, bsize, nblocks, me);
        else shmem_int_get(loc, sym, bsize * nblocks, me);
        local_read(kind, got, loc);
        expect(exp, sym, tst, sst, bsize, nblocks);
        snprintf(what, sizeof(what), "%s local %d tst %ld sst %ld bsize %zu nblocks %zu",
                 form == 0 ? "iget" : form == 1 ? "ibget" : "get", kind, tst, sst, bsize, nblocks);
        compare(exp, got, what, where);
    }
    local_free(kind, loc);
}

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    void *base = NULL;
    const size_t reg = sosx_data_segment(&base);
    const int registered = reg && (char *) sym_static >= (char *) base &&
                           (char *) (sym_static + N) <= (char *) base + reg;
    int *heap = shmem_malloc(N * sizeof(int));
    /* (tst, sst, bsize, nblocks): single elements, small blocks, blocks of >= 16 B at both
       kinds of offsets, abutting blocks (the contiguous forms) */
    static const long shapes[][4] = {{3, 1, 1, 1000}, {2, 5, 1, 700}, {5, 7, 3, 500}, {40, 36, 33, 100},
                                     {64, 128, 40, 30}, {16, 16, 16, 200}};
    for (int kind = 0; kind < 3; ++kind)
        for (size_t s = 0; s < sizeof(shapes) / sizeof(shapes[0]); ++s) {
            run(sym_static, "static data", kind, shapes[s][0], shapes[s][1], (size_t) shapes[s][2], (size_t) shapes[s][3]);
            run(heap, "host heap", kind, shapes[s][0], shapes[s][1], (size_t) shapes[s][2], (size_t) shapes[s][3]);
        }
    shmem_barrier_all();
    shmem_free(heap);
    if (!bad)
        printf("rma_static: PE %d/%d OK (%d checks, data segment %s)\n", me, np, checks,
               registered ? "registered" : "pageable");
    fflush(stdout);
    shmem_finalize();
    return bad != 0;
}
