// lock_checks.cpp -- what the distributed locks decide on plain data: the argument check
// (sos_lock_check) over the layout struct of sos_rma_check, and the texts of the two ways a
// lock call can end the job -- a wait that ran out, a lock word that holds no PE id + 1.
// No HIP and no runtime state: the file compiles with a plain C++ compiler.
#include <stdio.h>

#include "api_internal.h"

using namespace sosrt;

#define REFUSE(code, ...)                            \
    do {                                             \
        if (msg && n) snprintf(msg, n, __VA_ARGS__); \
        return code;                                 \
    } while (0)

// SOS's order (src/lock_c.c:44-65): SHMEM_ERR_CHECK_INITIALIZED, then
// SHMEM_ERR_CHECK_SYMMETRIC(lock, sizeof(long)); then this library's own.  Nothing here
// depends on my_pe: PE 0, the home of `last`, refuses what every other PE refuses.
extern "C" int sos_lock_check(const sos_rma_layout *l, const sos_lock_op *op, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    if (!l->initialized) REFUSE(SOS_RMA_NOT_INITIALIZED, "library not initialized");
    const uintptr_t p = (uintptr_t)op->lock;
    const sos_rma_region *reg = rma_find_region(l, p);
    if (!reg) REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"lock\" is not symmetric (%p)", op->lock);
    if (sizeof(long) > reg->size - (p - reg->base))
        REFUSE(SOS_RMA_NOT_SYMMETRIC, "Argument \"lock\" [%p..%p) exceeds %s [%p..%p)", op->lock,
               (const void *)(p + sizeof(long)), rma_region_name(reg->kind), (const void *)reg->base,
               (const void *)(reg->base + reg->size));
    // this library's own
    if (p % sizeof(long))
        REFUSE(SOS_RMA_BAD_TYPE_SIZE, "Argument \"lock\" (%p) must be aligned to 8 bytes", op->lock);
    if (l->n_pes == 1) return SOS_RMA_OK;
    if (reg->kind != SOS_RMA_REGION_DEVICE_HEAP)
        REFUSE(SOS_RMA_PEER_NOT_DEVICE_HEAP, "Argument \"lock\" (%p) is in this PE's %s: a lock shared by %d PEs "
               "needs the device symmetric heap (shmemx_malloc_device), the only memory mapped across PEs",
               op->lock, rma_region_name(reg->kind), l->n_pes);
    if (!l->mapped)
        REFUSE(SOS_RMA_NO_PATH, "No path to peer (the PEs' device heaps are not mapped: SHMEMX_TRANSPORT=p2p or "
               "both maps them)");
    return SOS_RMA_OK;
}

#undef REFUSE

extern "C" void sos_lock_expiry_message(const char *fn, const void *lock, int awaited, uint32_t data, double seconds,
                                        char *msg, size_t n)
{
    if (!msg || !n) return;
    snprintf(msg, n, "%s: lock %p not %s after %.0f s (SHMEMX_P2P_TIMEOUT): awaited %s in this PE's data half, "
             "last value seen 0x%08x (next = %u, signal = %u)", fn, lock,
             awaited == SOS_LOCK_AWAIT_SIGNAL ? "granted" : "handed over", seconds,
             awaited == SOS_LOCK_AWAIT_SIGNAL ? "SIGNAL (bit 31) from the predecessor"
                                              : "NEXT (bits 0-30) from the successor",
             data, data & 0x7FFFFFFFu, data >> 31);
}

extern "C" void sos_lock_corrupt_message(const void *lock, int value, int n_pes, char *msg, size_t n)
{
    if (!msg || !n) return;
    snprintf(msg, n, "lock word at %p is not a lock (last/next = %d, n_pes = %d): was it zero-initialised?", lock,
             value, n_pes);
}
