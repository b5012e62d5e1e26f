// onesided.cpp -- the host plumbing that put / get (rma.cpp), the atomics (amo.cpp),
// put-with-signal and the waits (signal.cpp), the locks (lock.cpp) and the contexts
// (ctx.cpp) share, each piece written once; onesided.h says what each does.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "onesided.h"
#include "runtime.h"

extern "C" char __data_start[] __attribute__((weak));
extern "C" char _end[] __attribute__((weak));

namespace sosrt {

bool heap_mapped(const State &s)
{
    if (!s.p2p_ready || s.peer_heap.size() != (size_t)s.n_pes) return false;
    for (char *b : s.peer_heap)
        if (!b) return false;
    return true;
}

void rma_layout_now(RmaLayout &out)
{
    State &s = st();
    auto add = [&](const void *b, size_t n, int kind) {
        if (b && n) out.regions.push_back({(uintptr_t)b, n, kind});
    };
    // the executable's data segment, as is_symmetric has it
    const char *data = __data_start && _end ? __data_start : nullptr;
    const size_t data_bytes = data ? (size_t)(_end - __data_start) : 0;
    add(s.dev_heap.base, s.dev_heap.size, SOS_RMA_REGION_DEVICE_HEAP);
    add(s.host_heap.base, s.host_heap.size, SOS_RMA_REGION_HOST_HEAP);
    add(data, data_bytes, SOS_RMA_REGION_DATA);
    for (auto &kv : s.dev_allocs) add(kv.first, kv.second, SOS_RMA_REGION_DEVICE_ALLOC);
    out.l = {s.initialized && !s.finalized, s.my_pe, s.n_pes, heap_mapped(s), (int)out.regions.size(),
             out.regions.data()};
}

void refused(const char *fn, const char *msg) { raise_error("%s: %s", fn, msg); }

char *translate(const void *remote, int pe)
{
    State &s = st();
    if (pe == s.my_pe) return (char *)remote;
    return s.peer_heap[(size_t)pe] + ((const char *)remote - s.peer_heap[(size_t)s.my_pe]);
}

void before_peer_read(Ctx &c, int pe, const char *fn)
{
    if (pe == st().my_pe) return;
    if (c.acq_pending) hip_check(acquire_system(c), fn);  // on the stream that does the read
    note_peer_read(c, false);
}

void after_peer_wait(hipStream_t stream, const char *fn)
{
    if (st().n_pes <= 1 || !st().p2p_ready) return;
    note_peer_wait();
    hip_check(acquire_system(stream), fn);
}

char *device_view(const void *p, size_t bytes)
{
    if (is_device_ptr(p)) return (char *)p;
    hipPointerAttribute_t a, z;
    if (hipPointerGetAttributes(&a, p) != hipSuccess ||
        hipPointerGetAttributes(&z, (const char *)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    const bool host = a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged;
    if (!host || z.type != a.type || !a.devicePointer || !z.devicePointer) return nullptr;
    // one mapping over the whole extent
    if ((char *)z.devicePointer - (char *)a.devicePointer != (ptrdiff_t)(bytes - 1)) return nullptr;
    return (char *)a.devicePointer;
}

void Pinned::reserve(size_t want, hipStream_t stream, const char *tag, const char *fn)
{
    if (want <= bytes) return;
    if (host) {
        hip_check(sync_system(stream), fn);
        release();
    }
    char what[64];
    snprintf(what, sizeof(what), "hipHostMalloc(%s)", tag);
    hip_check(hipHostMalloc(&host, want, hipHostMallocDefault), what);
    snprintf(what, sizeof(what), "hipHostGetDevicePointer(%s)", tag);
    hip_check(hipHostGetDevicePointer(&dev, host, 0), what);
    bytes = want;
}

void Pinned::release()
{
    if (host) (void)hipHostFree(host);
    host = dev = nullptr;
    bytes = 0;
}

}  // namespace sosrt
