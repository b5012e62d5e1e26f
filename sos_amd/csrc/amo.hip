// amo.hip -- one atomic memory operation on a 4- or 8-byte word: the device side of
// shmem_<T>_atomic_* (amo.cpp).
//
// One workgroup of one wave; lane 0 performs ONE read-modify-write (or an atomic load) at
// system scope on the word, which may be this PE's HBM, a peer's HBM mapped through the
// device heap, or host memory HIP allocated or registered (its device view).  The
// operation is the hardware's: an exchange for SET / SWAP, a compare-exchange for CSWAP,
// fetch_add / and / or / xor, an atomic load for FETCH.  There is no loop and no wait on
// memory anywhere.
//
// Float and double reach this file as the same-width integer's bit pattern and may only
// SET / FETCH / SWAP: no float arithmetic exists, so NaN payloads and -0 pass unchanged.
//
// Where the old value is wanted it is written to *fetch with a plain vector store.  What
// makes that store visible to its reader (the host, or a copy engine) is the stream's next
// system-scope release marker (release_system / sync_system, runtime.h), which every
// completion in amo.cpp and every quiet, fence and barrier issues; the kernel carries no
// fence of its own.
#include "elementwise.h"

namespace sos {

template <int W> struct AmoWord;
template <> struct AmoWord<4> { using type = uint32_t; };
template <> struct AmoWord<8> { using type = uint64_t; };

template <int W, int OP, bool FETCH>
__global__ __launch_bounds__(64) void k_amo(typename AmoWord<W>::type *target, typename AmoWord<W>::type value,
                                            typename AmoWord<W>::type cond, typename AmoWord<W>::type *fetch)
{
    using T = typename AmoWord<W>::type;
    if (threadIdx.x != 0) return;
    T old;
    if constexpr (OP == SOSX_AMO_SET || OP == SOSX_AMO_SWAP) {
        old = __hip_atomic_exchange(target, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if constexpr (OP == SOSX_AMO_FETCH) {
        old = __hip_atomic_load(target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if constexpr (OP == SOSX_AMO_CSWAP) {
        old = cond;  // receives the word's value when the comparison fails
        __hip_atomic_compare_exchange_strong(target, &old, value, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM);
    } else if constexpr (OP == SOSX_AMO_ADD) {
        old = __hip_atomic_fetch_add(target, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if constexpr (OP == SOSX_AMO_AND) {
        old = __hip_atomic_fetch_and(target, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if constexpr (OP == SOSX_AMO_OR) {
        old = __hip_atomic_fetch_or(target, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        static_assert(OP == SOSX_AMO_XOR, "unknown atomic operation");
        old = __hip_atomic_fetch_xor(target, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if constexpr (FETCH) *fetch = old;
}

}  // namespace sos

using namespace sos;

namespace {

template <int W, int OP, bool FETCH>
int launch(void *target, uint64_t value, uint64_t cond, void *fetch, hipStream_t st)
{
    using T = typename AmoWord<W>::type;
    hipLaunchKernelGGL((k_amo<W, OP, FETCH>), dim3(1), dim3(64), 0, st, (T *)target, (T)value, (T)cond, (T *)fetch);
    return hip_ok(hipGetLastError());
}

template <int W, int OP> int launch_fetch(void *target, uint64_t value, uint64_t cond, void *fetch, hipStream_t st)
{
    return fetch ? launch<W, OP, true>(target, value, cond, fetch, st)
                 : launch<W, OP, false>(target, value, cond, fetch, st);
}

template <int W> int launch_op(int op, void *target, uint64_t value, uint64_t cond, void *fetch, hipStream_t st)
{
    switch (op) {
        case SOSX_AMO_SET: return launch_fetch<W, SOSX_AMO_SET>(target, value, cond, fetch, st);
        case SOSX_AMO_FETCH: return launch<W, SOSX_AMO_FETCH, true>(target, value, cond, fetch, st);
        case SOSX_AMO_SWAP: return launch_fetch<W, SOSX_AMO_SWAP>(target, value, cond, fetch, st);
        case SOSX_AMO_CSWAP: return launch_fetch<W, SOSX_AMO_CSWAP>(target, value, cond, fetch, st);
        case SOSX_AMO_ADD: return launch_fetch<W, SOSX_AMO_ADD>(target, value, cond, fetch, st);
        case SOSX_AMO_AND: return launch_fetch<W, SOSX_AMO_AND>(target, value, cond, fetch, st);
        case SOSX_AMO_OR: return launch_fetch<W, SOSX_AMO_OR>(target, value, cond, fetch, st);
        case SOSX_AMO_XOR: return launch_fetch<W, SOSX_AMO_XOR>(target, value, cond, fetch, st);
        default: return SOSX_ERR_ARG;
    }
}

}  // namespace

extern "C" int sosx_amo(int op, void *target, uint64_t value, uint64_t cond, void *fetch, size_t width,
                        int is_float, void *stream)
{
    // every argument is checked before any device work
    if (width != 4 && width != 8) return SOSX_ERR_ARG;
    if (op < SOSX_AMO_SET || op > SOSX_AMO_XOR) return SOSX_ERR_ARG;
    if (is_float && op != SOSX_AMO_SET && op != SOSX_AMO_FETCH && op != SOSX_AMO_SWAP) return SOSX_ERR_OP;
    if (!target || (uintptr_t)target % width) return SOSX_ERR_ARG;
    if ((uintptr_t)fetch % width) return SOSX_ERR_ARG;
    if (op == SOSX_AMO_FETCH && !fetch) return SOSX_ERR_ARG;  // a load with nowhere to put it
    return width == 4 ? launch_op<4>(op, target, value, cond, fetch, as_stream(stream))
                      : launch_op<8>(op, target, value, cond, fetch, as_stream(stream));
}
