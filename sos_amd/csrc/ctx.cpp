// ctx.cpp -- communication contexts: shmem_ctx_create / destroy / quiet / fence,
// shmem_team_create_ctx, shmem_ctx_get_team, and the per-context halves of the runtime's
// ordering state.
//
// A context is an ordering domain with its own completion, and a HIP stream is exactly
// that.  Each context owns what two streams must not share: the stream, the system-scope
// release event (two streams recording one event overwrite each other's record), the
// pack / unpack stage, the nbi atomics' fetch ring, put-with-signal's ticket word and the
// "acquire owed" flag (runtime.h, struct Ctx).  The operations themselves are rma.cpp's,
// amo.cpp's and signal.cpp's, handed the context.
//
//  * SHMEM_CTX_DEFAULT is State::def_ctx over the library stream; it follows
//    shmemx_set_stream.  The non-ctx API, shmem_quiet, shmem_fence, the barriers and the
//    collectives use it and complete it alone: they do not drain created contexts.
//  * created contexts take non-blocking streams from a pool of SHMEMX_CTX_STREAMS
//    (default 3: with the library stream that fills the four hardware queues a process
//    opens), round-robin; contexts beyond the pool share a stream, which over-orders but is
//    correct -- a quiet on one may also complete a neighbour's work.
//  * shmem_ctx_quiet: the system-scope release and the stream synchronisation
//    (sync_system) on that context's stream only.  shmem_ctx_fence is the same call:
//    nothing weaker is shown to order the copy engine's deliveries.
//  * options are stored and returned; the library is not thread-multiple, so PRIVATE,
//    SERIALIZED and NOSTORE change nothing else.
//  * a handle is looked up, never dereferenced (sos_ctx_check, onesided_checks.cpp).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "onesided.h"
#include "runtime.h"
#include "sosx.h"

shmem_ctx_t SHMEM_CTX_DEFAULT = nullptr;

namespace sosrt {

namespace {

inline shmem_ctx_t ctx_handle(Ctx *c) { return reinterpret_cast<shmem_ctx_t>(c); }

hipStream_t pool_stream(State &s, int slot)
{
    if (s.ctx_pool.empty()) {
        char msg[256];
        const int k = sos_ctx_pool_size(getenv("SHMEMX_CTX_STREAMS"), msg, sizeof(msg));
        if (k < 0) raise_error("%s", msg);
        s.ctx_streams = k;
        s.ctx_pool.assign((size_t)k, nullptr);
    }
    hipStream_t &q = s.ctx_pool[(size_t)slot];
    if (!q) hip_check(hipStreamCreateWithFlags(&q, hipStreamNonBlocking), "hipStreamCreate(context)");
    return q;
}

// quiet, then give back what the context owns (not its pool stream)
void destroy(State &s, Ctx *c)
{
    hip_check(sync_system(*c), "shmem_ctx_destroy");
    if (c->sys_ev) (void)hipEventDestroy(c->sys_ev);
    if (c->stage) (void)hipFree(c->stage);
    if (c->amo_ring) (void)hipFree(c->amo_ring);
    if (c->ticket) (void)hipFree(c->ticket);
    s.ctxs.erase(std::remove(s.ctxs.begin(), s.ctxs.end(), c), s.ctxs.end());
    if (s.ctx_dead.size() >= 64) s.ctx_dead.erase(s.ctx_dead.begin());
    s.ctx_dead.push_back(c);
    delete c;
}

int create(Team *team, long options, shmem_ctx_t *out, const char *fn)
{
    State &s = st();
    if (out) *out = SHMEM_CTX_INVALID;
    char msg[256];
    if (sos_ctx_options_check(options, msg, sizeof(msg)) != SOS_CTX_OK) {
        warn("%s: %s", fn, msg);
        return 1;
    }
    if (!out) {
        warn("%s: Argument \"ctx\" is NULL", fn);
        return 1;
    }
    if (s.ctx_pool.empty()) (void)pool_stream(s, 0);  // reads SHMEMX_CTX_STREAMS
    Ctx *c = new Ctx;
    c->options = options;
    c->team = team;
    c->t_start = team->start;
    c->t_stride = team->stride;
    c->t_size = team->size;
    c->slot = sos_ctx_stream_slot(s.ctx_created++, s.ctx_streams);
    c->stream = pool_stream(s, c->slot);
    // a wait for a peer before the context existed says nothing about its stream
    c->acq_pending = s.n_pes > 1 && s.p2p_ready;
    s.ctxs.push_back(c);
    s.ctx_dead.erase(std::remove(s.ctx_dead.begin(), s.ctx_dead.end(), (const void *)c), s.ctx_dead.end());
    *out = ctx_handle(c);
    return 0;
}

}  // namespace

Ctx &default_ctx()
{
    State &s = st();
    s.def_ctx.is_default = true;
    s.def_ctx.stream = s.stream;
    s.def_ctx.t_start = 0;
    s.def_ctx.t_stride = 1;
    s.def_ctx.t_size = s.n_pes;
    s.def_ctx.team = &s.world;
    return s.def_ctx;
}

Ctx &ctx_checked(shmem_ctx_t handle, int *pe, const char *fn)
{
    State &s = st();
    if (!s.initialized || s.finalized) raise_error("%s: library not initialized", fn);
    Ctx &d = default_ctx();
    static std::vector<sos_ctx_entry> live;
    live.clear();
    live.push_back({&d, d.t_start, d.t_stride, d.t_size});
    for (Ctx *c : s.ctxs) live.push_back({c, c->t_start, c->t_stride, c->t_size});
    const sos_ctx_table table = {(int)live.size(), live.data(), (int)s.ctx_dead.size(), s.ctx_dead.data()};
    char msg[256];
    int index = -1;
    if (sos_ctx_check(&table, handle, pe, &index, msg, sizeof(msg)) != SOS_CTX_OK) raise_error("%s: %s", fn, msg);
    return index == 0 ? d : *s.ctxs[(size_t)index - 1];
}

hipError_t release_system(Ctx &c)
{
    ++c.releases;
    if (c.is_default) return release_system(c.stream);
    if (!c.sys_ev) {
        const hipError_t e = hipEventCreateWithFlags(&c.sys_ev, hipEventReleaseToSystem | hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    ++st().sys_releases;
    return hipEventRecord(c.sys_ev, c.stream);
}

hipError_t sync_system(Ctx &c)
{
    hipError_t e;
    if (c.is_default) {
        ++c.releases;
        e = sync_system(c.stream);
    } else {
        e = release_system(c);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    }
    ++c.syncs;
    c.completed = c.enqueued;
    return e;
}

hipError_t acquire_system(Ctx &c)
{
    if (c.is_default) return acquire_system(c.stream);
    State &s = st();
    if (!s.acq_mask) {
        // once: zeroed before any stream's acquire kernel may touch it
        hipError_t e = hipMalloc(&s.acq_mask, sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(s.acq_mask, 0, sizeof(unsigned), c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess) return e;
    }
    ++s.sys_acquires;
    ++s.acquire_kernels;
    c.acq_pending = false;
    return sosx_acquire_system(s.acq_mask, c.stream) == SOSX_OK ? hipSuccess : hipErrorLaunchFailure;
}

void note_peer_read(Ctx &c, bool own_acquire)
{
    State &s = st();
    ++s.peer_reads;
    if (own_acquire) ++s.sys_acquires;
    else if (c.acq_pending) ++s.peer_reads_unacquired;
}

void *stage(Ctx &c, size_t bytes)
{
    if (c.is_default) return stage(bytes);
    if (bytes <= c.stage_bytes && c.stage) return c.stage;
    if (c.stage) {
        hip_check(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
        hip_check(hipFree(c.stage), "hipFree");
        c.stage = nullptr;
    }
    const size_t sz = bytes < (1u << 20) ? (1u << 20) : bytes;
    hip_check(hipMalloc(&c.stage, sz), "hipMalloc(context stage)");
    c.stage_bytes = sz;
    return c.stage;
}

void ctx_destroy_team(Team *t)
{
    State &s = st();
    const std::vector<Ctx *> all = s.ctxs;
    for (Ctx *c : all)
        if (c->team == t && !(c->options & SHMEM_CTX_PRIVATE)) destroy(s, c);
}

void ctx_destroy_all()
{
    State &s = st();
    while (!s.ctxs.empty()) destroy(s, s.ctxs.back());
    for (hipStream_t &q : s.ctx_pool)
        if (q) (void)hipStreamDestroy(q);
    s.ctx_pool.clear();
    s.ctx_dead.clear();
}

}  // namespace sosrt

using namespace sosrt;

// The entries behind shmem_ctx_create ... shmem_ctx_get_team (ctx_gen.cpp, libsos_amd_ctx.so).
extern "C" {

int sos_api_ctx_create(long options, shmem_ctx_t *ctx)
{
    check_initialized("shmem_ctx_create");
    return create(&st().world, options, ctx, "shmem_ctx_create");
}

int sos_api_team_create_ctx(shmem_team_t team, long options, shmem_ctx_t *ctx)
{
    // src/teams_c.c4:150-164
    check_initialized("shmem_team_create_ctx");
    if (team == SHMEM_TEAM_INVALID) {
        if (ctx) *ctx = SHMEM_CTX_INVALID;
        return -1;
    }
    Team *t = team_from_handle(team);
    if (!t->valid) raise_error("shmem_team_create_ctx: invalid team");
    return create(t, options, ctx, "shmem_team_create_ctx");
}

int sos_api_ctx_get_team(shmem_ctx_t ctx, shmem_team_t *team)
{
    // src/teams_c.c4:166-178
    check_initialized("shmem_ctx_get_team");
    if (ctx == SHMEM_CTX_INVALID) {
        if (team) *team = SHMEM_TEAM_INVALID;
        return -1;
    }
    Ctx &c = ctx_checked(ctx, nullptr, "shmem_ctx_get_team");
    if (team) *team = team_handle(c.team);
    return 0;
}

void sos_api_ctx_destroy(shmem_ctx_t ctx)
{
    // src/contexts_c.c:53-71
    check_initialized("shmem_ctx_destroy");
    if (ctx == SHMEM_CTX_INVALID) return;
    Ctx &c = ctx_checked(ctx, nullptr, "shmem_ctx_destroy");
    if (c.is_default) raise_error("shmem_ctx_destroy(): SHMEM_CTX_DEFAULT cannot be destroyed");
    destroy(st(), &c);
}

void sos_api_ctx_quiet(shmem_ctx_t ctx)
{
    hip_check(sync_system(ctx_checked(ctx, nullptr, "shmem_ctx_quiet")), "shmem_ctx_quiet");
}

// As strong as shmem_fence, which is shmem_quiet: see the head of this file.
void sos_api_ctx_fence(shmem_ctx_t ctx)
{
    hip_check(sync_system(ctx_checked(ctx, nullptr, "shmem_ctx_fence")), "shmem_ctx_fence");
}

// How many pool streams created contexts share (SHMEMX_CTX_STREAMS as read at the first
// creation; the default before that).
int sosx_ctx_streams(void) { return st().ctx_streams; }

#ifdef SOSX_TEST_HOOKS
// Test build only (tests/test_gpu_ctx_multipe.py): what the library did on one context --
// out[0] its stream as a number, [1] its pool slot (-1: the library stream), [2] operations
// enqueued, [3] of those completed by a synchronisation of ITS stream, [4] records of its
// release event, [5] host waits for its stream.
int sosx_ctx_stats(shmem_ctx_t ctx, long long out[6])
{
    Ctx &c = ctx_checked(ctx, nullptr, "sosx_ctx_stats");
    out[0] = (long long)(uintptr_t)c.stream;
    out[1] = c.slot;
    out[2] = c.enqueued;
    out[3] = c.completed;
    out[4] = c.releases;
    out[5] = c.syncs;
    return 0;
}
#endif

}  // extern "C"
