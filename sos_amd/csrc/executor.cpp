// executor.cpp -- owns the execution of a per-PE plan (plan.h) for one collective call:
// operand placement (execute), the transports' executors and the phase profiler.  Which
// plan a call runs is the API layer's choice (api.cpp op_to_all, SOS's AUTO rule).
//
// Executors:
//   * RCCL (exec_rccl): each round's transfers are ncclSend/ncclRecv (byte views) inside
//     one ncclGroupStart/End on the PE's stream, followed by the round's fused folds
//     (sosx_fold) on the same stream -- no host round trip until the call returns.
//   * peer-to-peer (execute_p2p -> p2p.cpp): the receiver reads the sender's HBM.
//   * the striped host ring (striped_host_ring): host-resident ring reductions cut into
//     stripes that pipeline H2D, exchange and D2H over either transport.
// Host-resident source/target are staged through device memory (H2D, device
// reduction, D2H), as the north star's host-symmetric-heap path.
#include "executor.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "dtypes.h"
#include "sosx.h"

using namespace sosrt;
using sosplan::Plan;

namespace {

// ---------------------------------------------------------------------------------
// optional per-phase timing (sosx_prof_*), HIP events on the PE stream
// ---------------------------------------------------------------------------------
struct Prof {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> fold_ev, xfer_ev;
    size_t nf = 0, nx = 0;
    double fold_ms = 0, xfer_ms = 0, call_ms = 0;
    long nfold = 0, nxfer = 0, ncall = 0;
    hipEvent_t get(std::vector<std::pair<hipEvent_t, hipEvent_t>> &v, size_t &n, bool second)
    {
        if (!second) {
            if (n == v.size()) {
                hipEvent_t a, b;
                (void)hipEventCreate(&a);
                (void)hipEventCreate(&b);
                v.push_back({a, b});
            }
            return v[n].first;
        }
        return v[n++].second;
    }
    void collect()
    {
        (void)hipStreamSynchronize(sosrt::st().stream);  // every event of the call complete
        for (size_t i = 0; i < nf; ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, fold_ev[i].first, fold_ev[i].second) == hipSuccess) fold_ms += ms;
        }
        for (size_t i = 0; i < nx; ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, xfer_ev[i].first, xfer_ev[i].second) == hipSuccess) xfer_ms += ms;
        }
        nfold += (long)nf;
        nxfer += (long)nx;
        nf = nx = 0;
    }
};
Prof g_prof;

}  // namespace

namespace sosrt {

void prof_mark(int which, bool end, hipStream_t s)
{
    if (!g_prof.on) return;
    auto &v = which == 0 ? g_prof.fold_ev : g_prof.xfer_ev;
    auto &n = which == 0 ? g_prof.nf : g_prof.nx;
    (void)hipEventRecord(g_prof.get(v, n, end), s);
}

void prof_call_done()
{
    if (!g_prof.on) return;
    g_prof.ncall++;
    g_prof.collect();
}

int run_locals(const sosplan::Round &r, const Bufs &b, int op, int dt, hipStream_t stream)
{
    for (const auto &l : r.ops) {
        if (l.kind == sosplan::COPY) {
            if (b.at(l.in_buf[0], l.in_off[0]) == b.at(l.out_buf, l.out_off)) continue;
            hipError_t e = hipMemcpyAsync(b.wat(l.out_buf, l.out_off), b.at(l.in_buf[0], l.in_off[0]),
                                          l.count, hipMemcpyDefault, stream);
            if (e != hipSuccess) return SOSX_ERR_HIP;
            continue;
        }
        if (l.kind == sosplan::ZERO) {
            if (hipMemsetAsync(b.wat(l.out_buf, l.out_off), 0, l.count, stream) != hipSuccess)
                return SOSX_ERR_HIP;
            continue;
        }
        const void *ins[sosplan::PLAN_MAX_PE];
        for (int k = 0; k < l.nin; ++k) ins[k] = b.at(l.in_buf[k], l.in_off[k]);
        prof_mark(0, false, stream);
        int rc;
        if (l.kind == sosplan::PREFIX) {
            void *outs[sosplan::PLAN_MAX_PE];
            for (int k = 0; k < l.nout; ++k) outs[k] = b.wat(l.outs_buf[k], l.outs_off[k]);
            rc = sosx_prefix(op, dt, outs, ins, l.nin, l.own, l.count, stream);
        } else {
            rc = sosx_fold(op, dt, l.order, b.wat(l.out_buf, l.out_off), ins, l.nin, l.count, stream);
        }
        prof_mark(0, true, stream);
        if (rc) return rc;
    }
    return SOSX_OK;
}

const char *status_text(int rc)
{
    switch (rc) {
        case SOSX_ERR_DTYPE: return "invalid data type";
        case SOSX_ERR_OP: return "unsupported reduction for this data type";
        case SOSX_ERR_UNSUPPORTED: return "long double reductions are not supported on the gfx950 device path";
        case SOSX_ERR_HIP: return "HIP runtime failure";
        case SOSX_ERR_RCCL: return "RCCL failure";
        default: return "invalid argument";
    }
}

}  // namespace sosrt

namespace {

// Is round r, for this PE of the WORLD team, a pure allgather of equal chunks inside
// DST: one send of this PE's chunk (bytes B at off0 + me*B) to every other PE and one
// receive of PE q's chunk at off0 + q*B from every PE q, no local ops?  (The ring and
// recdbl_direct plans' second round when P divides nreduce.)  Then RCCL's own
// allgather moves exactly the bytes the send/receive pairs would.  A collect's uneven
// round never passes: every transfer must carry the same byte count at owner * bytes, which
// for a collect holds only when all P lengths are equal (a zero length drops transfers,
// so the count of 2(P-1) fails first).
bool allgather_round(const sosplan::Round &r, const Team &t, uint64_t *off0, uint64_t *B)
{
    const State &s = st();
    const int P = t.size, me = t.my_idx;
    if (P < 2 || t.start != 0 || t.stride != 1 || P != s.n_pes || !r.ops.empty() ||
        r.xfers.size() != 2 * (size_t)(P - 1))
        return false;
    uint64_t bytes = 0, base = 0;
    bool have = false;
    std::vector<char> sent((size_t)P, 0), got((size_t)P, 0);
    for (const auto &x : r.xfers) {
        if (x.buf != sosplan::DST || x.peer == me || x.peer < 0 || x.peer >= P) return false;
        const int owner = x.send ? me : x.peer;
        if (!have) {
            bytes = x.bytes;
            if (!bytes || x.off < (uint64_t)owner * bytes) return false;
            base = x.off - (uint64_t)owner * bytes;
            have = true;
        }
        if (x.bytes != bytes || x.off != base + (uint64_t)owner * bytes) return false;
        char &seen = (x.send ? sent : got)[(size_t)x.peer];
        if (seen) return false;
        seen = 1;
    }
    *off0 = base;
    *B = bytes;
    return true;
}

// RCCL executor: one ncclGroup per round, folds after it, all on `stream`.
int exec_rccl(const Plan &p, const Team &t, const Bufs &b, int op, int dt, hipStream_t stream)
{
    State &s = st();
    for (const auto &r : p.rounds) {
        uint64_t off0 = 0, B = 0;
        if (s.rccl_allgather && allgather_round(r, t, &off0, &B)) {
            prof_mark(1, false, stream);
            char *base = b.wat(sosplan::DST, off0);
            if (ncclAllGather(base + (size_t)t.my_idx * B, base, B, ncclUint8, s.comm, stream) != ncclSuccess)
                return SOSX_ERR_RCCL;
            prof_mark(1, true, stream);
            continue;
        }
        if (!r.xfers.empty()) {
            prof_mark(1, false, stream);
            if (ncclGroupStart() != ncclSuccess) return SOSX_ERR_RCCL;
            for (const auto &x : r.xfers) {
                const int peer = t.world_rank(x.peer);
                ncclResult_t rc = x.send
                    ? ncclSend(b.at(x.buf, x.off), x.bytes, ncclUint8, peer, s.comm, stream)
                    : ncclRecv(b.wat(x.buf, x.off), x.bytes, ncclUint8, peer, s.comm, stream);
                if (rc != ncclSuccess) {
                    (void)ncclGroupEnd();
                    return SOSX_ERR_RCCL;
                }
            }
            if (ncclGroupEnd() != ncclSuccess) return SOSX_ERR_RCCL;
            prof_mark(1, true, stream);
        }
        int rc = run_locals(r, b, op, dt, stream);
        if (rc) return rc;
    }
    return SOSX_OK;
}

// SHMEMX_RCCL_ALLREDUCE (sosx_set_rccl_allreduce): may this reduction run as one
// ncclAllReduce?  Only over a world-shaped team (the communicator is the world's) and
// only where RCCL's type and op give the combine's own element semantics: integer
// sum/prod/min/max of 8/32/64-bit kinds (dtypes.h: char, ptrdiff_t and the unsigned
// types included) are the same in any order -- two's-complement wrap, min/max with the
// kind's signedness -- so mode 1 stays bit-exact; mode 2 adds fp32/fp64 sum/prod, whose
// bits follow RCCL's order instead of SOS's (DESIGN.md section 5 tolerance).  No RCCL
// type for 16-bit integers, no bitwise ops, no complex or long double: those keep their
// SOS schedule.
bool rccl_allreduce_type(const Team &t, int op, int dt, ncclDataType_t *ty, ncclRedOp_t *ro)
{
    const State &s = st();
    if (!s.rccl_allreduce || !s.comm || s.transport != TRANSPORT_RCCL || t.start != 0 ||
        t.stride != 1 || t.size != s.n_pes)
        return false;
    switch (op) {
        case SOSX_OP_SUM: *ro = ncclSum; break;
        case SOSX_OP_PROD: *ro = ncclProd; break;
        case SOSX_OP_MIN: *ro = ncclMin; break;
        case SOSX_OP_MAX: *ro = ncclMax; break;
        default: return false;
    }
    const bool fp_ok = s.rccl_allreduce >= 2 && (op == SOSX_OP_SUM || op == SOSX_OP_PROD);
    switch (sos_dtype_info(dt).kind) {
        case K_S8: *ty = ncclInt8; return true;
        case K_U8: *ty = ncclUint8; return true;
        case K_S32: *ty = ncclInt32; return true;
        case K_U32: *ty = ncclUint32; return true;
        case K_S64: *ty = ncclInt64; return true;
        case K_U64: *ty = ncclUint64; return true;
        case K_F32: *ty = ncclFloat32; return fp_ok;
        case K_F64: *ty = ncclFloat64; return fp_ok;
        default: return false;
    }
}

// Plan cache: the same call shape every step reuses its plan.
// A collect's plan is a function of the P byte lengths `lens` as well (empty otherwise).
const Plan &cached_plan(int alg, int P, int me, uint64_t count, uint64_t ts, unsigned smis,
                        unsigned dmis, const uint64_t *lens = nullptr)
{
    static std::map<std::tuple<int, int, int, uint64_t, uint64_t, unsigned, unsigned,
                               std::vector<uint64_t>>, Plan> cache;
    auto key = std::make_tuple(alg, P, me, count, ts, smis, dmis,
                               lens ? std::vector<uint64_t>(lens, lens + P) : std::vector<uint64_t>());
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (cache.size() > 64) cache.clear();
    Plan p;
    if (sosplan::build(alg, P, me, count, ts, smis, dmis, &p, lens) != SOSX_OK)
        raise_error("internal: cannot build reduction plan (alg %d, P %d)", alg, P);
    return cache.emplace(key, std::move(p)).first->second;
}

// The peer-to-peer leg of execute(): operands in the IPC-mapped heap run in place,
// others are staged through the stage region; scan scratch follows the staged operand.
void execute_p2p(const Plan &p, const Team &t, int alg, size_t count, size_t ts, const void *source,
                 void *target, const char *dsrc, char *ddst, bool direct, size_t base, int op,
                 int dt, const char *fn, const uint64_t *lens = nullptr)
{
    State &s = st();
    const char *hb = s.sym_stage;
    if (!direct && p.reads_src && p.src_bytes)
        hip_check(hipMemcpyAsync(s.sym_stage, source, p.src_bytes, hipMemcpyDefault, s.stream), "stage in");
    char *scr = nullptr;
    size_t scr_off = 0;
    if (p.scratch_bytes && p.scr_sent) {
        scr = s.sym_stage + base;
        scr_off = base;
    } else if (p.scratch_bytes) {
        scr = (char *)scratch(p.scratch_bytes);
    }
    const unsigned smis = (unsigned)((uintptr_t)dsrc & 15), dmis = (unsigned)((uintptr_t)ddst & 15);
    P2PBufs pb{dsrc, ddst, scr, (size_t)(dsrc - hb), (size_t)(ddst - hb), scr_off, smis, dmis};
    int rc = p2p_exec(p, t, alg, count, ts, pb, op, dt, s.stream, lens);
    if (rc) raise_error("%s: %s", fn, status_text(rc));
    // p2p_exec returned with the stream drained; a staged result still has to come out
    // (its target may be pageable memory: a full stream synchronisation)
    if (!direct && p.writes_dst) {
        hip_check(hipMemcpyAsync(target, ddst, p.dst_bytes, hipMemcpyDefault, s.stream), "stage out");
        hip_check(sync_system(s.stream), fn);
    }
    prof_call_done();
}

// Host-resident ring reductions, pipelined in stripes.
//
// SOS's operands live in the host symmetric heap.  Staged whole, a call costs
// H2D(n*s) + exchange + D2H(n*s) in sequence.  The ring's element order depends only on
// which ring chunk an element is in (chunk c is folded starting at PE c,
// src/collectives.c:693-727), so the vector is cut into stripes that take the k-th
// slice of EVERY ring chunk: stripe k = concat over c of chunk c's elements
// [k*L, k*L + L_k).  Run as an ordinary ring over its P*L_k elements, the stripe's chunk c
// is exactly that slice of the full chunk c, owned and folded by PE c in the same order,
// so the result is bit-identical to the ring over the whole vector (tests/test_stripes.py
// checks this with the oracle).  The r = n mod P last elements of chunks c < r form a
// final stripe of r elements (one per chunk: again the ring's own split).  Stripes flow
// through three device slots:
//   H2D(k+2) on a copy stream || exchange(k) on the library stream || D2H(k-1),
// so a call approaches max(H2D, D2H) on a full-duplex PCIe link instead of their sum.
// Returns false (nothing done) when the call does not qualify.
bool striped_host_ring(int alg, void *target, const void *source, size_t count, size_t ts,
                       const Team &t, int op, int dt, const char *fn)
{
    State &s = st();
    const int P = t.size;
    if (alg != SOSX_ALG_RING || P < 2 || P > SOSX_MAX_FOLD || s.host_stripe_bytes == 0) return false;
    const size_t q = count / (size_t)P, r = count % (size_t)P;
    // Stripe shape, from measurements of this copy pattern on MI355X with HIP 7.0
    // (tools/diag/stripe_copy_probe.py, profiles/r2_stripe_probe.txt): with 2-D copies a
    // 512 MiB pass takes 0.62x the serial time at 8-16 stripes, a 64 MiB pass 0.72x even
    // with 0.5 MiB slices.  So: slices of >= SHMEMX_HOST_STRIPE_BYTES (default 256 KiB),
    // at most 16 stripes.  The p2p executor synchronises the host every round, which
    // leaves the copy streams little to overlap: it stripes only when
    // SHMEMX_HOST_STRIPE_BYTES is set explicitly (the tests use tiny stripes to exercise
    // the decomposition).
    const bool p2p = s.transport == TRANSPORT_P2P;
    if (p2p && !s.host_stripe_explicit) return false;
    size_t L = (s.host_stripe_bytes + ts - 1) / ts;
    if (!s.host_stripe_explicit) L = std::max(L, (q + 15) / 16);
    if (p2p) {  // three slots in the IPC-mapped stage region
        const size_t lim = s.sym_stage_bytes / 3 / ((size_t)P * ts);
        if (lim < L) L = lim;
    }
    if (L == 0 || q < 2 * L) return false;
    // only now the (costlier) residency queries: both operands must be host memory
    if (is_device_ptr(source) || is_device_ptr(target)) return false;
    const size_t slot_bytes = align256((size_t)P * L * ts);
    char *slots;
    if (p2p) {
        slots = s.sym_stage;
    } else {
        if (s.stripes_bytes < 3 * slot_bytes) {
            if (s.stripes) {
                hip_check(hipStreamSynchronize(s.stream), "hipStreamSynchronize");
                hip_check(hipFree(s.stripes), "hipFree(stripes)");
                s.stripes = nullptr;
            }
            hip_check(hipMalloc(&s.stripes, 3 * slot_bytes), "hipMalloc(stripes)");
            s.stripes_bytes = 3 * slot_bytes;
        }
        slots = (char *)s.stripes;
    }
    if (!s.pipe_h2d) {
        hip_check(hipStreamCreateWithFlags(&s.pipe_h2d, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipStreamCreateWithFlags(&s.pipe_d2h, hipStreamNonBlocking), "hipStreamCreate");
        for (auto &slot : s.pipe_ev)
            for (hipEvent_t &e : slot)
                hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToSystem), "hipEventCreate");
    }
    enum { H2D = 0, XCH = 1, D2H = 2 };
    const size_t nfull = (q + L - 1) / L;
    const size_t nstripes = nfull + (r ? 1 : 0);
    debug_msg("%s: host-resident ring in %zu stripes of %zu x %zu elements", fn, nstripes,
              (size_t)P, L);
    auto disp = [&](size_t c) { return c * q + (c < r ? c : r); };
    // stripe k: slice length per chunk, first element of the slice within each chunk,
    // and the number of chunks it takes a slice of
    auto geom = [&](size_t k, size_t *len, size_t *first, size_t *npieces) {
        if (k < nfull) {
            *first = k * L;
            *len = q - k * L < L ? q - k * L : L;
            *npieces = (size_t)P;
        } else {
            *first = q;
            *len = 1;
            *npieces = r;
        }
    };
    const char *src = (const char *)source;
    char *dst = (char *)target;
    // The np slices of a stripe, packed in the slot at len-element spacing, sit in the
    // host vector at ring-chunk spacing: (q+1) elements for chunks c < r, q after.  So a
    // stripe moves as at most two 2-D copies (hipMemcpy2DAsync), not np 1-D ones: the
    // runtime pipelines a few large rectangular copies well and many small 1-D copies
    // badly (profiles/r2_stripe_probe.txt).
    auto copy_slices = [&](char *slot, char *host, size_t first, size_t len, size_t np,
                           bool to_dev, hipStream_t strm) {
        const size_t lo = np < r ? np : r;  // slices of the longer chunks, then the others
        const size_t groups[2][2] = {{0, lo}, {lo, np}};
        for (const auto &g : groups) {
            const size_t c0 = g[0], rows = g[1] - g[0];
            if (!rows) continue;
            const size_t hpitch = (c0 < r ? q + 1 : q) * ts;
            char *h = host + (disp(c0) + first) * ts;
            char *d = slot + c0 * len * ts;
            const hipError_t e =
                to_dev ? hipMemcpy2DAsync(d, len * ts, h, hpitch, len * ts, rows,
                                          hipMemcpyHostToDevice, strm)
                       : hipMemcpy2DAsync(h, hpitch, d, len * ts, len * ts, rows,
                                          hipMemcpyDeviceToHost, strm);
            hip_check(e, to_dev ? "stripe H2D" : "stripe D2H");
        }
    };
    auto h2d = [&](size_t k) {
        const int sl = (int)(k % 3);
        size_t len, first, np;
        geom(k, &len, &first, &np);
        char *slot = slots + (size_t)sl * slot_bytes;
        hip_check(hipStreamWaitEvent(s.pipe_h2d, s.pipe_ev[sl][D2H], 0), "stripe wait");
        copy_slices(slot, (char *)src, first, len, np, true, s.pipe_h2d);
        hip_check(hipEventRecord(s.pipe_ev[sl][H2D], s.pipe_h2d), "stripe event");
    };
    // every slot starts free: its "D2H done" event is recorded on the idle copy stream
    for (auto &slot : s.pipe_ev) hip_check(hipEventRecord(slot[D2H], s.pipe_d2h), "stripe event");
    h2d(0);
    if (nstripes > 1) h2d(1);
    for (size_t k = 0; k < nstripes; ++k) {
        if (k + 2 < nstripes) h2d(k + 2);
        const int sl = (int)(k % 3);
        size_t len, first, np;
        geom(k, &len, &first, &np);
        const size_t m = len * np;  // elements of this stripe's ring
        char *slot = slots + (size_t)sl * slot_bytes;
        hip_check(hipStreamWaitEvent(s.stream, s.pipe_ev[sl][H2D], 0), "stripe wait");
        const unsigned mis = (unsigned)((uintptr_t)slot & 15);
        const Plan &p = cached_plan(SOSX_ALG_RING, P, t.my_idx, m, ts, mis, mis);
        char *scr = p.scratch_bytes ? (char *)scratch(p.scratch_bytes) : nullptr;
        int rc;
        if (p2p) {
            const size_t off = (size_t)(slot - s.sym_stage);
            P2PBufs pb{slot, slot, scr, off, off, 0, mis, mis};
            rc = p2p_exec(p, t, SOSX_ALG_RING, m, ts, pb, op, dt, s.stream);
        } else {
            Bufs b{slot, slot, scr};
            rc = exec_rccl(p, t, b, op, dt, s.stream);
        }
        if (rc) raise_error("%s: %s", fn, status_text(rc));
        hip_check(hipEventRecord(s.pipe_ev[sl][XCH], s.stream), "stripe event");
        hip_check(hipStreamWaitEvent(s.pipe_d2h, s.pipe_ev[sl][XCH], 0), "stripe wait");
        copy_slices(slot, dst, first, len, np, false, s.pipe_d2h);
        hip_check(hipEventRecord(s.pipe_ev[sl][D2H], s.pipe_d2h), "stripe event");
    }
    hip_check(sync_system(s.pipe_d2h), fn);
    hip_check(sync_system(s.stream), fn);
    prof_call_done();
    return true;
}

}  // namespace

namespace sosrt {

void execute(int alg, void *target, const void *source, size_t count, size_t ts, const Team &t,
             int op, int dt, const char *fn, bool reduction, const uint64_t *lens)
{
    State &s = st();
    // operand extents: count * ts for both, except fcollect's target and alltoall's operands
    // and a collect's own length and the sum of all
    uint64_t sb64 = 0, db64 = 0, maxlen = 0;
    const bool collect = sosplan::is_collect(alg);
    if (collect) {
        sb64 = lens[t.my_idx];
        for (int q = 0; q < t.size; ++q) {
            db64 += lens[q];
            maxlen = std::max(maxlen, lens[q]);
        }
    } else if (sosplan::extents(alg, t.size, count, ts, &sb64, &db64) != SOSX_OK)
        raise_error("%s: operand size overflows (count %zu, element size %zu, %d PEs)", fn, count, ts, t.size);
    const size_t src_bytes = (size_t)sb64, dst_bytes = (size_t)db64;
    const size_t bytes = count * ts;
    // fcollect, alltoall and collect receive into target blocks while peers still read the
    // source: staged, their target never shares the source's bytes
    const bool split = sosplan::never_in_place(alg);
    ncclDataType_t ar_ty = ncclUint8;
    ncclRedOp_t ar_op = ncclSum;
    const bool ar = reduction && rccl_allreduce_type(t, op, dt, &ar_ty, &ar_op);
    if (!ar && striped_host_ring(alg, target, source, count, ts, t, op, dt, fn)) return;
    if (s.transport == TRANSPORT_P2P) {
        // buffers must live in the IPC-mapped device heap; anything else is staged
        // through this PE's stage region, whose offset is published: in place for the
        // reductions, scans and broadcasts; a split target is staged behind the source
        // (every target byte is written: no stage-in of the target)
        const char *hb = s.sym_stage;
        auto in_heap = [&](const void *p, size_t n) {
            return hb && (const char *)p >= hb && (const char *)p + n <= hb + s.dev_heap_bytes;
        };
        const bool direct = in_heap(source, src_bytes) && in_heap(target, dst_bytes);
        // (a collect's target sits behind the LONGEST contribution, so that the fit test
        // below sees the same size on every PE)
        const size_t doff = split ? align256(collect ? (size_t)maxlen : src_bytes) : 0;
        const char *dsrc = direct ? (const char *)source : s.sym_stage;
        char *ddst = direct ? (char *)target : s.sym_stage + doff;
        const unsigned smis = (unsigned)((uintptr_t)dsrc & 15), dmis = (unsigned)((uintptr_t)ddst & 15);
        const Plan &p = cached_plan(alg, t.size, t.my_idx, count, ts, smis, dmis, lens);
        // the staged operand and the scratch the peers read (scan results) must fit the
        // IPC-mapped stage region; the decision depends only on sizes, residency of
        // symmetric addresses and SHMEMX_STAGE_BYTES, so every PE takes the same branch
        const size_t staged = direct ? 0 : (split ? doff + dst_bytes : bytes);
        const size_t base = align256(staged);
        const size_t need = (p.scratch_bytes && p.scr_sent) ? base + p.scratch_bytes : staged;
        if (need <= s.sym_stage_bytes) {
            execute_p2p(p, t, alg, count, ts, source, target, dsrc, ddst, direct, base, op, dt, fn, lens);
            return;
        }
        if (!s.comm)
            raise_error("%s: %zu bytes (staged operand + exchange scratch) exceed the p2p stage "
                        "region (SHMEMX_STAGE_BYTES=%zu); allocate operands with "
                        "shmemx_malloc_device or raise SHMEMX_STAGE_BYTES", fn, need,
                        s.sym_stage_bytes);
        // both transports are up: this call runs on RCCL instead
        debug_msg("%s: %zu bytes exceed the p2p stage region, call runs on RCCL", fn, need);
    }

    // residency: device pointers run in place; host memory is staged through HBM
    const bool dev_src = is_device_ptr(source);
    const bool dev_dst = target == source ? dev_src : is_device_ptr(target);
    const char *dsrc = (const char *)source;
    char *ddst = (char *)target;
    char *stg = nullptr;
    const size_t half = align256(src_bytes);
    if (!dev_src || !dev_dst) {
        stg = (char *)stage(half + align256(dst_bytes));
        if (!dev_src) dsrc = stg;
        if (!dev_dst) ddst = target == source && !split ? stg : stg + half;
    }
    if (ar) {
        if (!dev_src) hip_check(hipMemcpyAsync(stg, source, bytes, hipMemcpyHostToDevice, s.stream), "H2D");
        prof_mark(1, false, s.stream);
        if (ncclAllReduce(dsrc, ddst, count, ar_ty, ar_op, s.comm, s.stream) != ncclSuccess)
            raise_error("%s: %s", fn, status_text(SOSX_ERR_RCCL));
        prof_mark(1, true, s.stream);
        if (!dev_dst)
            hip_check(hipMemcpyAsync(target, ddst, bytes, hipMemcpyDeviceToHost, s.stream), "D2H");
        hip_check(sync_system(s.stream), fn);
        prof_call_done();
        return;
    }
    const Plan &p = cached_plan(alg, t.size, t.my_idx, count, ts, (unsigned)((uintptr_t)dsrc & 15),
                                (unsigned)((uintptr_t)ddst & 15), lens);
    if (!dev_src && p.reads_src && p.src_bytes)
        hip_check(hipMemcpyAsync(stg, source, p.src_bytes, hipMemcpyHostToDevice, s.stream), "H2D");
    Bufs b{dsrc, ddst, p.scratch_bytes ? (char *)scratch(p.scratch_bytes) : nullptr};
    const int rc = exec_rccl(p, t, b, op, dt, s.stream);
    if (rc) raise_error("%s: %s", fn, status_text(rc));
    if (!dev_dst && p.writes_dst)
        hip_check(hipMemcpyAsync(target, ddst, p.dst_bytes, hipMemcpyDeviceToHost, s.stream), "D2H");
    hip_check(sync_system(s.stream), fn);
    prof_call_done();
}

}  // namespace sosrt

// ---- phase timing -----------------------------------------------------------------
extern "C" {

void sosx_prof_enable(int on)
{
    g_prof.on = on != 0;
    g_prof.fold_ms = g_prof.xfer_ms = 0;
    g_prof.nfold = g_prof.nxfer = g_prof.ncall = 0;
}

void sosx_prof_get(double *fold_ms, double *xfer_ms, long *nfold, long *nxfer, long *ncall)
{
    if (fold_ms) *fold_ms = g_prof.fold_ms;
    if (xfer_ms) *xfer_ms = g_prof.xfer_ms;
    if (nfold) *nfold = g_prof.nfold;
    if (nxfer) *nxfer = g_prof.nxfer;
    if (ncall) *ncall = g_prof.ncall;
}

}  // extern "C"
