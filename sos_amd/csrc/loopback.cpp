// loopback.cpp -- owns the single-GPU loopback team (sosx_loopback_allreduce,
// sosx_loopback_collect) used by the tests and bench.py: P PEs' buffers on one GPU, the
// plans' transfers as device-to-device copies matched in the same FIFO-per-peer order
// RCCL uses, the local operations through the executors' run_locals (executor.h).
#include <hip/hip_runtime.h>

#include <deque>
#include <map>
#include <vector>

#include "dtypes.h"
#include "executor.h"
#include "plan.h"
#include "sosx.h"

using namespace sosrt;
using sosplan::Plan;

// Run the P plans over srcs/dsts/scr (scr[p] owned: freed here) with device-to-device
// copies as the transport, matched FIFO per ordered pair as RCCL matches.
static int run_loopback(const std::vector<Plan> &plans, void *const *srcs, void *const *dsts,
                        std::vector<void *> &scr, int op, int datatype, hipStream_t sm)
{
    const int P = (int)plans.size();
    int rc;
    struct Send { const char *ptr; uint64_t bytes; int from; };
    std::map<std::pair<int, int>, std::deque<Send>> q;  // (from, to) FIFO, as RCCL matches
    std::vector<size_t> k(P, 0);
    std::vector<int> posted(P, 0), outstanding(P, 0);
    std::vector<std::vector<char>> recv_done(P);
    auto bufs = [&](int p) { return Bufs{(const char *)srcs[p], (char *)dsts[p], (char *)scr[p]}; };
    auto free_scr = [&] { for (auto v : scr) if (v) (void)hipFree(v); };
    for (;;) {
        bool progress = false, all_done = true;
        for (int p = 0; p < P; ++p) {
            if (k[p] >= plans[p].rounds.size()) continue;
            all_done = false;
            const auto &r = plans[p].rounds[k[p]];
            const Bufs b = bufs(p);
            if (!posted[p]) {
                for (const auto &x : r.xfers)
                    if (x.send) {
                        q[{p, x.peer}].push_back(Send{b.at(x.buf, x.off), x.bytes, p});
                        outstanding[p]++;
                    }
                recv_done[p].assign(r.xfers.size(), 0);
                posted[p] = 1;
                progress = true;
            }
            bool recvs_ok = true;
            for (size_t i = 0; i < r.xfers.size(); ++i) {
                const auto &x = r.xfers[i];
                if (x.send || recv_done[p][i]) continue;
                auto &fifo = q[{x.peer, p}];
                // FIFO per (peer, me): only the oldest pending send from that peer matches
                bool earlier_pending = false;
                for (size_t j = 0; j < i; ++j)
                    if (!r.xfers[j].send && r.xfers[j].peer == x.peer && !recv_done[p][j]) earlier_pending = true;
                if (earlier_pending || fifo.empty()) {
                    recvs_ok = false;
                    continue;
                }
                Send snd = fifo.front();
                fifo.pop_front();
                if (snd.bytes != x.bytes) {
                    free_scr();
                    return SOSX_ERR_ARG;  // plan mismatch between PEs
                }
                if (hipMemcpyAsync(b.wat(x.buf, x.off), snd.ptr, x.bytes, hipMemcpyDeviceToDevice, sm) != hipSuccess)
                    return SOSX_ERR_HIP;
                outstanding[snd.from]--;
                recv_done[p][i] = 1;
                progress = true;
            }
            if (recvs_ok && outstanding[p] == 0) {
                rc = run_locals(r, b, op, datatype, sm);
                if (rc) return rc;
                k[p]++;
                posted[p] = 0;
                progress = true;
            }
        }
        if (all_done) break;
        if (!progress) {
            free_scr();
            return SOSX_ERR_ARG;  // deadlock: inconsistent plans
        }
    }
    hipError_t e = sync_system(sm);
    prof_call_done();
    free_scr();
    return e == hipSuccess ? SOSX_OK : SOSX_ERR_HIP;
}

extern "C" {

int sosx_loopback_allreduce(int alg, int P, int op, int datatype, void *const *srcs,
                            void *const *dsts, size_t count, void *stream)
{
    if (P < 1 || P > SOSX_MAX_FOLD || !srcs || !dsts) return SOSX_ERR_ARG;
    // broadcast, fcollect and alltoall move bytes: any sized type, no (op, type) rule;
    // srcs[p] and dsts[p] span the plan's extents (sosx_plan_extents)
    const bool moves = sosplan::is_bcast(alg) || sosplan::is_fcollect(alg) || sosplan::is_alltoall(alg);
    int rc = moves ? (sos_dtype_info(datatype).size ? SOSX_OK : SOSX_ERR_DTYPE)
                   : sos_check_op(op, datatype);
    if (rc) return rc;
    if (sosplan::is_bcast(alg) && ((alg - sosplan::PLAN_BCAST) >> 1) >= P) return SOSX_ERR_ARG;
    const size_t ts = sos_dtype_info(datatype).size;
    hipStream_t sm = (hipStream_t)stream;
    const int a = sosplan::resolve_alg(alg, count * ts, 16384);
    std::vector<Plan> plans(P);
    std::vector<void *> scr(P, nullptr);
    for (int p = 0; p < P; ++p) {
        rc = sosplan::build(a, P, p, count, ts, (unsigned)((uintptr_t)srcs[p] & 15),
                            (unsigned)((uintptr_t)dsts[p] & 15), &plans[p]);
        if (rc) return rc;
        if (plans[p].scratch_bytes && hipMalloc(&scr[p], plans[p].scratch_bytes) != hipSuccess)
            return SOSX_ERR_HIP;
    }
    return run_loopback(plans, srcs, dsts, scr, op, datatype, sm);
}

int sosx_loopback_collect(int P, void *const *srcs, void *const *dsts, const size_t *lens, void *stream)
{
    if (P < 1 || P > sosplan::PLAN_MAX_PE || !srcs || !dsts || !lens) return SOSX_ERR_ARG;
    uint64_t l64[sosplan::PLAN_MAX_PE];
    for (int p = 0; p < P; ++p) l64[p] = lens[p];
    std::vector<Plan> plans(P);
    std::vector<void *> scr(P, nullptr);
    for (int p = 0; p < P; ++p) {
        const int rc = sosplan::build_collect(P, p, l64, &plans[p]);
        if (rc) return rc;
        if ((lens[p] && !srcs[p]) || (plans[p].dst_bytes && !dsts[p])) return SOSX_ERR_ARG;
    }
    return run_loopback(plans, srcs, dsts, scr, SOSX_OP_SUM, SOSX_DT_UCHAR, (hipStream_t)stream);
}

}  // extern "C"
