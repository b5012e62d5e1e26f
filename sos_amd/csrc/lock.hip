// lock.hip -- the non-waiting part of shmem_set_lock, shmem_test_lock and shmem_clear_lock
// as ONE launch each: the device side of lock.cpp.
//
// One workgroup of one wave; lane 0 runs one step function of lock_proto.h (enqueue,
// try_acquire, release or hand_off) over system-scope atomics: a short dependent chain of two to four
// operations on 32-bit words that may be this PE's HBM, a peer's HBM mapped through the
// device heap, or host memory HIP allocated or registered (its device view).  Which peer's
// word the chain touches is known only from the values it reads, so the kernel gets the
// table of every PE's base (device memory) and the lock's offset, and the step checks every
// such value against 1..n_pes before it forms an address from it.
//
// There is no loop and no wait on memory anywhere: a step that would have to wait returns a
// status instead (LOCK_QUEUED, LOCK_PENDING) and lock.cpp probes from the host.
//
// The result record goes to *result with plain vector stores.  What makes it visible to the
// host is the stream's next system-scope release marker (sync_system, runtime.h), as for
// the atomics' old values (amo.hip).
//
// Memory order: the read-modify-writes are system-scope releases, so the zero this PE stores
// into its own data half is visible before `last` names the PE, and a release kernel's
// compare-and-swap or hand-off publishes nothing before the critical section's stores.  The
// acquire half is the host's: acquire_system on the stream after the kernel (lock.cpp).
#define SOS_LOCK_FN __host__ __device__ inline
#include "elementwise.h"
#include "lock_proto.h"

namespace sos {

struct DeviceAtomics {
    __device__ static void store(uint32_t *p, uint32_t v)
    {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __device__ static uint32_t load(uint32_t *p)
    {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __device__ static uint32_t exchange(uint32_t *p, uint32_t v)
    {
        return __hip_atomic_exchange(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __device__ static uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v)
    {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELEASE, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM);
        return expect;  // the word's value either way
    }
    __device__ static uint32_t fetch_or(uint32_t *p, uint32_t v)
    {
        return __hip_atomic_fetch_or(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
};

template <int KIND>
__global__ __launch_bounds__(64) void k_lock_step(uint32_t *last, uint32_t *my_data, const uint64_t *table,
                                                  uint64_t offset, int me, int n_pes, soslock::Result *result)
{
    if (threadIdx.x != 0) return;
    soslock::Result r;
    if constexpr (KIND == soslock::LOCK_ENQUEUE) {
        r = soslock::enqueue<DeviceAtomics>(last, my_data, table, offset, me, n_pes);
    } else if constexpr (KIND == soslock::LOCK_TRY) {
        r = soslock::try_acquire<DeviceAtomics>(last, my_data, me, n_pes);
    } else if constexpr (KIND == soslock::LOCK_RELEASE) {
        r = soslock::release<DeviceAtomics>(last, my_data, table, offset, me, n_pes);
    } else {
        static_assert(KIND == soslock::LOCK_HANDOFF, "unknown lock step");
        r = soslock::hand_off<DeviceAtomics>(my_data, table, offset, n_pes, 0);
    }
    *result = r;
}

}  // namespace sos

using namespace sos;

namespace {

template <int KIND>
int launch(uint32_t *last, uint32_t *my_data, const uint64_t *table, uint64_t offset, int me, int n_pes,
           soslock::Result *result, hipStream_t st)
{
    hipLaunchKernelGGL((k_lock_step<KIND>), dim3(1), dim3(64), 0, st, last, my_data, table, offset, me, n_pes, result);
    return hip_ok(hipGetLastError());
}

}  // namespace

extern "C" int sosx_lock_step(int kind, void *last_word, void *my_data_word, const uint64_t *table, uint64_t offset,
                              int me, int n_pes, void *result, void *stream)
{
    // every argument is checked before any device work
    if (kind < SOSX_LOCK_ENQUEUE || kind > SOSX_LOCK_HANDOFF) return SOSX_ERR_ARG;
    if (!last_word || (uintptr_t)last_word % 4) return SOSX_ERR_ARG;
    if (!my_data_word || (uintptr_t)my_data_word % 4) return SOSX_ERR_ARG;
    if (!table || (uintptr_t)table % 8 || offset % 4) return SOSX_ERR_ARG;
    if (!result || (uintptr_t)result % 8) return SOSX_ERR_ARG;
    if (n_pes < 1 || me < 0 || me >= n_pes) return SOSX_ERR_ARG;
    static_assert(sizeof(soslock::Result) == SOSX_LOCK_RESULT_BYTES, "the record's size is part of the C ABI");
    uint32_t *last = (uint32_t *)last_word, *mine = (uint32_t *)my_data_word;
    soslock::Result *res = (soslock::Result *)result;
    hipStream_t st = as_stream(stream);
    switch (kind) {
        case SOSX_LOCK_ENQUEUE: return launch<soslock::LOCK_ENQUEUE>(last, mine, table, offset, me, n_pes, res, st);
        case SOSX_LOCK_TRY: return launch<soslock::LOCK_TRY>(last, mine, table, offset, me, n_pes, res, st);
        case SOSX_LOCK_RELEASE: return launch<soslock::LOCK_RELEASE>(last, mine, table, offset, me, n_pes, res, st);
        default: return launch<soslock::LOCK_HANDOFF>(last, mine, table, offset, me, n_pes, res, st);
    }
}
