// executor.h -- what the API layer (api.cpp), the loopback (loopback.cpp) and the
// peer-to-peer transport (p2p.cpp) use of the plan executors (executor.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "plan.h"
#include "runtime.h"

namespace sosrt {

// Phase timing (sosx_prof_*): mark the start/end of a fold (which = 0) or a transfer
// (which = 1) on stream s; a no-op while the profiler is off.
void prof_mark(int which, bool end, hipStream_t s);

// The rest is internal to the library: kept out of its dynamic symbol table.
#pragma GCC visibility push(hidden)

// One collective call is over (its work queued on the library stream): count it and
// fold its marks into the totals.  A no-op while the profiler is off.
void prof_call_done();

constexpr size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// The three buffers a plan names (plan.h Buf), as addresses on this PE.
struct Bufs {
    const char *src;
    char *dst;
    char *scr;
    const char *at(int b, uint64_t off) const
    {
        return (b == sosplan::SRC ? src : b == sosplan::DST ? (const char *)dst : (const char *)scr) + off;
    }
    char *wat(int b, uint64_t off) const { return (char *)at(b, off); }
};

// Run one round's local operations.
int run_locals(const sosplan::Round &r, const Bufs &b, int op, int dt, hipStream_t stream);

// Run plan `alg` (a reduction SOSX_ALG_*, a scan or a broadcast, plan.h) for this PE
// over team t, on the library stream; returns when the call is complete.  `reduction`:
// the call may take the ncclAllReduce path (rccl_allreduce_type).  `lens`: PLAN_COLLECT's P
// byte lengths (count and ts are not used then).
void execute(int alg, void *target, const void *source, size_t count, size_t ts, const Team &t,
             int op, int dt, const char *fn, bool reduction = false, const uint64_t *lens = nullptr);

const char *status_text(int rc);

#pragma GCC visibility pop

}  // namespace sosrt
