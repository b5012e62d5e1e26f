/*
 * lock_static_pe.c -- shmem_set_lock / shmem_test_lock / shmem_clear_lock on a single PE with
 * the lock in STATIC data and on the host symmetric heap (tools/oshrun -np 1; built by
 * tests/test_gpu_lock_multipe.py).
 *
 * Static data is kernel-reachable only where shmem_init registered the data segment with
 * HIP; under SHMEMX_REGISTER_DATA=0 it is pageable host memory: the library completes its
 * stream and runs the lock's steps on the host.  Either way a taken lock refuses
 * shmem_test_lock, a cleared one grants it, and the word is zero whenever nobody holds it.
 * Prints "lock_static: PE 0/1 OK (<k> checks, data segment <registered|pageable>)".
 */
#include <shmem.h>
#include <shmemx.h>
#include <stdio.h>
#include <string.h>

static long s_lock[2];
static long s_counter;

static int checks, bad;

#define EXPECT(want, got, what)                                                               \
    do {                                                                                      \
        ++checks;                                                                             \
        const long long w_ = (long long) (want), g_ = (long long) (got);                      \
        if (w_ != g_ && !bad++)                                                               \
            fprintf(stderr, "lock_static: %s (%s): %lld, expected %lld\n", what, where, g_, w_); \
    } while (0)

static void run(long *lock, long *counter, const char *where)
{
    const int me = shmem_my_pe();
    EXPECT(0, *lock, "the lock before its first use");
    for (int k = 0; k < 5; ++k) {
        shmem_set_lock(lock);
        EXPECT(me + 1, *lock & 0xFFFFFFFFl, "last while held");
        EXPECT(1, shmem_test_lock(lock), "test_lock on a held lock");
        shmem_long_atomic_inc(counter, me);
        shmem_clear_lock(lock);
        EXPECT(0, *lock, "the lock after clear_lock");
    }
    for (int k = 0; k < 5; ++k) {
        EXPECT(0, shmem_test_lock(lock), "test_lock on a free lock");
        shmem_long_atomic_inc(counter, me);
        shmem_clear_lock(lock);
        EXPECT(0, *lock, "the lock after test_lock and clear_lock");
    }
    shmem_quiet();
    EXPECT(10, *counter, "counter");
}

int main(void)
{
    shmem_init();
    const int me = shmem_my_pe(), np = shmem_n_pes();
    if (np != 1) {
        fprintf(stderr, "lock_static: run with one PE (locks across PEs need the device heap)\n");
        shmem_finalize();
        return 2;
    }
    void *base = NULL;
    const size_t reg = sosx_data_segment(&base);
    const int registered = reg && (char *) s_lock >= (char *) base && (char *) (s_lock + 2) <= (char *) base + reg;
    long *heap = shmem_malloc(64);
    memset(heap, 0, 64);
    run(&s_lock[1], &s_counter, "static data");
    run(heap, heap + 4, "host heap");
    shmem_free(heap);
    if (!bad)
        printf("lock_static: PE %d/%d OK (%d checks, data segment %s)\n", me, np, checks,
               registered ? "registered" : "pageable");
    fflush(stdout);
    shmem_finalize();
    return bad != 0;
}
