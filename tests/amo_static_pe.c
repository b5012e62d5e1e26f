/*
 * amo_static_pe.c -- atomic memory operations with the calling PE as the target and the word
 * in STATIC data or on the host symmetric heap (one process per PE, tools/oshrun; built by
 * tests/test_gpu_amo_multipe.py).
 *
 * Static data is kernel-reachable only where shmem_init registered the data segment with
 * HIP; under SHMEMX_REGISTER_DATA=0 it is pageable host memory, which only this process
 * can address: the library completes its stream and does the operation on the host.  Either
 * way every form must return the old value and leave the new one, which the host reads
 * where it lies.  Prints "amo_static: PE <i>/<n> OK (<k> checks, data segment
 * <registered|pageable>)".
 */
#include <shmem.h>
#include <shmemx.h>
#include <limits.h>
#include <stdio.h>
#include <string.h>

static long s_long[4];
static int s_int[4];
static uint64_t s_u64[4];
static uint32_t s_u32[4];
static float s_float[2];
static double s_double[2];

static int checks, bad;

#define EXPECT(want, got, what)                                                              \
    do {                                                                                     \
        ++checks;                                                                            \
        const long long w_ = (long long) (want), g_ = (long long) (got);                     \
        if (w_ != g_ && !bad++)                                                              \
            fprintf(stderr, "amo_static: %s (%s): %lld, expected %lld\n", what, where, g_, w_); \
    } while (0)

static uint32_t fbits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static uint64_t dbits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static float bits_f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static double bits_d(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }

static void run(long *l, int *i, uint64_t *u64, uint32_t *u32, float *f, double *d, const char *where)
{
    const int me = shmem_my_pe();
    /* the AMO forms on long and int */
    l[0] = 10;
    EXPECT(10, shmem_long_atomic_fetch_add(&l[0], 5, me), "fetch_add old");
    EXPECT(15, shmem_long_atomic_fetch_inc(&l[0], me), "fetch_inc old");
    shmem_long_atomic_add(&l[0], -20, me);
    shmem_long_atomic_inc(&l[0], me);
    shmem_quiet();
    EXPECT(-3, l[0], "word after add and inc");
    EXPECT(-3, shmem_long_atomic_compare_swap(&l[0], -3, 99, me), "compare_swap hit old");
    EXPECT(99, shmem_long_atomic_compare_swap(&l[0], -3, 7, me), "compare_swap miss old");
    EXPECT(99, l[0], "word after a missed compare_swap");
    i[1] = INT_MAX;
    EXPECT(INT_MAX, shmem_int_atomic_fetch_add(&i[1], 1, me), "int wrap old");
    EXPECT(INT_MIN, shmem_int_atomic_fetch(&i[1], me), "INT_MAX + 1");
    u64[1] = UINT64_MAX;
    EXPECT(UINT64_MAX, shmem_uint64_atomic_fetch_add(&u64[1], 2, me), "uint64 wrap old");
    EXPECT(1, u64[1], "UINT64_MAX + 2");
    /* the EXTENDED forms, floats as bits */
    EXPECT(99, shmem_long_atomic_swap(&l[0], 1234, me), "swap old");
    shmem_long_atomic_set(&l[0], 4321, me);
    EXPECT(4321, shmem_long_atomic_fetch(&l[0], me), "fetch after set");
    f[0] = -0.0f;
    EXPECT(0x80000000u, fbits(shmem_float_atomic_swap(&f[0], bits_f(0x7FC12345u), me)), "float swap old (-0)");
    EXPECT(0x7FC12345u, fbits(shmem_float_atomic_fetch(&f[0], me)), "float fetch (NaN payload)");
    d[1] = bits_d(0x7FF80000DEADBEEFull);
    EXPECT(0x7FF80000DEADBEEFull, dbits(shmem_double_atomic_swap(&d[1], -0.0, me)), "double swap old (NaN payload)");
    shmem_quiet();
    EXPECT(0x8000000000000000ull, dbits(d[1]), "double word (-0)");
    shmem_double_atomic_set(&d[0], 2.5, me);
    shmem_quiet();
    EXPECT(dbits(2.5), dbits(d[0]), "double set");
    /* the BITWISE forms */
    u32[0] = 0xFF00FF00u;
    EXPECT(0xFF00FF00u, shmem_uint32_atomic_fetch_and(&u32[0], 0x0FF00FF0u, me), "fetch_and old");
    EXPECT(0x0F000F00u, shmem_uint32_atomic_fetch_or(&u32[0], 0x000000FFu, me), "fetch_or old");
    EXPECT(0x0F000FFFu, shmem_uint32_atomic_fetch_xor(&u32[0], 0xFFFFFFFFu, me), "fetch_xor old");
    shmem_uint32_atomic_and(&u32[0], 0xFFFF0000u, me);
    shmem_uint32_atomic_or(&u32[0], 0x00000001u, me);
    shmem_uint32_atomic_xor(&u32[0], 0x80000000u, me);
    shmem_quiet();
    EXPECT(0x70FF0001u, u32[0], "word after and, or, xor");
    u64[0] = 0xF0F0F0F0F0F0F0F0ull;
    EXPECT(0xF0F0F0F0F0F0F0F0ull, shmem_uint64_atomic_fetch_xor(&u64[0], 0xFFFFFFFF00000000ull, me), "64-bit fetch_xor old");
    EXPECT(0x0F0F0F0FF0F0F0F0ull, u64[0], "64-bit word after xor");
    /* nbi forms: fetch in static data too; the old values are there after one quiet */
    l[1] = 100;
    shmem_long_atomic_fetch_add_nbi(&l[2], &l[1], 11, me);
    shmem_long_atomic_fetch_inc_nbi(&l[3], &l[1], me);
    shmem_quiet();
    EXPECT(100, l[2], "fetch_add_nbi old");
    EXPECT(111, l[3], "fetch_inc_nbi old");
    EXPECT(112, l[1], "word after the nbi forms");
    /* a burst with no sync in between */
    i[0] = 0;
    for (int k = 0; k < 100; ++k) shmem_int_atomic_add(&i[0], 3, me);
    shmem_quiet();
    EXPECT(300, i[0], "burst of 100 adds");
}

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    void *base = NULL;
    const size_t reg = sosx_data_segment(&base);
    const int registered = reg && (char *) s_long >= (char *) base && (char *) (s_long + 4) <= (char *) base + reg;
    char *heap = shmem_malloc(256);
    memset(heap, 0, 256);
    run(s_long, s_int, s_u64, s_u32, s_float, s_double, "static data");
    run((long *) heap, (int *) (heap + 32), (uint64_t *) (heap + 64), (uint32_t *) (heap + 96), (float *) (heap + 112),
        (double *) (heap + 128), "host heap");
    shmem_barrier_all();
    shmem_free(heap);
    if (!bad)
        printf("amo_static: PE %d/%d OK (%d checks, data segment %s)\n", me, np, checks,
               registered ? "registered" : "pageable");
    fflush(stdout);
    shmem_finalize();
    return bad != 0;
}
