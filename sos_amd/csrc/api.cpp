// api.cpp -- owns the SOS argument-check layer: every sos_api_* entry behind the generated
// typed bindings, the pshmem_*mem and 32/64 active-set forms with their weak aliases, and
// shmemx_reduce_local.  An entry runs SOS's checks in SOS's order, picks the schedule
// (op_to_all) and hands the call to the small shared-memory path (smallpath.cpp) or to
// the plan executors (executor.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "api_internal.h"
#include "dtypes.h"
#include "executor.h"
#include "plan.h"
#include "runtime.h"
#include "shmemx.h"
#include "sosx.h"

using namespace sosrt;

namespace {

// ---- the checks ------------------------------------------------------------------------

// SHMEM_ERR_CHECK_OVERLAP (src/shmem_internal.h:319-336), complete overlap allowed
void check_overlap(const void *a, const void *b, size_t bytes, const char *fn)
{
    if (a == b || bytes == 0) return;
    const char *lo = (const char *)(a < b ? a : b), *hi = (const char *)(a < b ? b : a);
    if (lo + bytes > hi)
        raise_error("%s: Argument \"dest\" [%p..%p) overlaps argument (%p)", fn, (const void *)lo,
                    (const void *)(lo + bytes), (const void *)hi);
}

void check_symmetric(const void *p, size_t bytes, const char *what, const char *fn)
{
    if (st().error_checking && bytes && !is_symmetric(p, bytes))
        raise_error("%s: argument \"%s\" (%p, %zu bytes) is not symmetric", fn, what, p, bytes);
}

// nelems * type_size for the size_t-count team forms: SOS multiplies unchecked; a count
// whose byte size does not fit size_t is refused instead of wrapping.
size_t checked_bytes(size_t nelems, size_t type_size, const char *what, const char *fn)
{
    if (type_size && nelems > SIZE_MAX / type_size)
        raise_error("%s: Argument %s (%zu) times the element size (%zu) overflows size_t", fn, what,
                    nelems, type_size);
    return nelems * type_size;
}

// SHMEM_ERR_CHECK_ACTIVE_SET (src/shmem_internal.h:214-227) for the deprecated active-set
// forms, whose stride is 1 << logPE_stride (src/collectives_c.c4:226).  SOS shifts
// without a check (undefined for logPE_stride >= 31 or < 0) and tests the last member
// with `> num_pes`; here both are refused: logPE_stride outside [0, 30], and a set whose
// last member is not a PE.  The extent is computed in 64 bits (no int overflow).
int active_set_stride(int PE_start, int logPE_stride, int PE_size, const char *fn)
{
    const State &s = st();
    if (logPE_stride < 0 || logPE_stride > 30)
        raise_error("%s: Invalid active set (PE_start = %d, logPE_stride = %d, PE_size = %d)", fn,
                    PE_start, logPE_stride, PE_size);
    const int stride = 1 << logPE_stride;
    const long long last = (long long)PE_start + (long long)(PE_size - 1) * stride;
    if (PE_start < 0 || PE_size < 0 || last >= s.n_pes)
        raise_error("%s: Invalid active set (PE_start = %d, PE_stride = %d, PE_size = %d)", fn,
                    PE_start, stride, PE_size);
    if (!(s.my_pe >= PE_start && s.my_pe <= last && (s.my_pe - PE_start) % stride == 0))
        raise_error("%s: Calling PE (%d) is not a member of the active set", fn, s.my_pe);
    return stride;
}

void check_member(const Team &t, const char *fn)
{
    if (t.my_idx < 0) raise_error("%s: calling PE is not a member of the team", fn);
}

// Team-relative root check shared by the broadcasts (SHMEM_ERR_CHECK_PE, then the
// root must be a member: src/collectives.c:435 real_root = PE_start + PE_root*stride).
void check_root(int PE_root, int size, const char *fn)
{
    if (PE_root < 0 || PE_root >= size)
        raise_error("%s: Invalid PE_root %d (team/active set of %d PEs)", fn, PE_root, size);
}

}  // namespace

// The helpers of this block sit inside extern "C": the library has always carried their
// unmangled names in its dynamic symbol table, and that table stays as it is.
extern "C" {
namespace {

// SHMEM_ERR_CHECK_OVERLAP for operands of different extents; complete overlap allowed
void check_overlap2(const void *dest, size_t db, const void *source, size_t sb, const char *fn)
{
    if (dest == source || !db || !sb) return;
    const char *d = (const char *)dest, *s = (const char *)source;
    if (d < s + sb && s < d + db)
        raise_error("%s: Argument \"dest\" [%p..%p) overlaps argument (%p)", fn, (const void *)d,
                    (const void *)(d + db), (const void *)s);
}

// SHMEM_ERR_CHECK_POSITIVE (src/shmem_internal.h:198-204)
void check_positive(ptrdiff_t v, const char *name, const char *fn)
{
    if (v <= 0) raise_error("%s: Argument %s must be positive (%ld)", fn, name, (long)v);
}

Team *checked_team(shmem_team_t team, const char *fn)
{
    Team *t = team_from_handle(team);
    if (!t || !t->valid) raise_error("%s: invalid team", fn);
    return t;
}

// The checked active set as a Team (the calling PE is a member).
Team active_set_team(int PE_start, int logPE_stride, int PE_size, const char *fn)
{
    const int stride = active_set_stride(PE_start, logPE_stride, PE_size, fn);
    Team t;
    t.start = PE_start;
    t.stride = stride;
    t.size = PE_size;
    t.my_idx = (st().my_pe - PE_start) / stride;
    t.valid = true;
    return t;
}

// es * ((n - 1) * stride + 1): the bytes a strided run of n >= 1 elements spans
size_t strided_extent(size_t n, ptrdiff_t stride, size_t es, const char *fn)
{
    const size_t span = checked_bytes(n - 1, (size_t)stride, "nelems", fn);
    if (span == SIZE_MAX) raise_error("%s: strided extent overflows size_t", fn);
    return checked_bytes(span + 1, es, "nelems", fn);
}

void check_team_size(const Team &t, const char *fn)
{
    if (t.size > sosplan::PLAN_MAX_PE)
        raise_error("%s: teams of more than %d PEs are not supported", fn, sosplan::PLAN_MAX_PE);
}

// ---- fcollect, alltoall, alltoalls (src/collectives.c:1284-1531) ------------------------
//
// Checks in SOS's order (src/collectives_c.c4:505-725), with two deliberate deviations
// (INTEGRATION.md): the symmetric and overlap checks cover the operands' TRUE extents
// (SOS checks nelems * size only), and every alltoalls form refuses a stride < 1 (SOS's
// team forms do not check).

void local_copy(void *dest, const void *source, size_t bytes, const char *fn)
{
    State &s = st();
    if (dest != source) hip_check(hipMemcpyAsync(dest, source, bytes, hipMemcpyDefault, s.stream), fn);
    hip_check(sync_system(s.stream), fn);
}

// The checked part shared by the team and active-set forms.  pSync (active-set forms) is
// only checked: it holds SHMEM_SYNC_VALUE on entry and is left so.
void fcollect_checked(const Team &t, void *dest, const void *source, size_t nelems, size_t es,
                      const long *pSync, const char *fn)
{
    const size_t sb = checked_bytes(nelems, es, "nelems", fn);
    const size_t db = checked_bytes(sb, (size_t)t.size, "nelems", fn);
    check_symmetric(dest, db, "dest", fn);
    check_symmetric(source, sb, "source", fn);
    if (pSync) check_symmetric(pSync, sizeof(long) * SHMEM_COLLECT_SYNC_SIZE, "pSync", fn);
    check_overlap2(dest, db, source, sb, fn);
    check_member(t, fn);
    if (nelems == 0) return;  // src/collectives.c:1351
    if (t.size == 1) return local_copy(dest, source, sb, fn);
    check_team_size(t, fn);
    execute(sosplan::PLAN_FCOLLECT, dest, source, nelems, es, t, SOSX_OP_SUM, SOSX_DT_UCHAR, fn);
}

void alltoall_checked(const Team &t, void *dest, const void *source, size_t nelems, size_t es,
                      const long *pSync, const char *fn)
{
    const size_t B = checked_bytes(nelems, es, "nelems", fn);
    const size_t bytes = checked_bytes(B, (size_t)t.size, "nelems", fn);
    check_symmetric(dest, bytes, "dest", fn);
    check_symmetric(source, bytes, "source", fn);
    if (pSync) check_symmetric(pSync, sizeof(long) * SHMEM_ALLTOALL_SYNC_SIZE, "pSync", fn);
    check_overlap2(dest, bytes, source, bytes, fn);
    check_member(t, fn);
    if (nelems == 0) return;  // src/collectives.c:1459
    if (t.size == 1) return local_copy(dest, source, bytes, fn);
    check_team_size(t, fn);
    execute(sosplan::PLAN_ALLTOALL, dest, source, nelems, es, t, SOSX_OP_SUM, SOSX_DT_UCHAR, fn);
}

// collect (src/collectives.c:1215-1276): every PE contributes its OWN nelems and the
// target holds the contributions in PE order.  No PE knows the others' lengths on entry
// (SOS runs a linear prefix over pSync); here the team first exchanges the byte lengths:
// in the headers of the small path's slots where the node shared segment exists
// (small_collect_exchange, which also carries the payloads of small calls), else by an
// internal PLAN_FCOLLECT of one uint64_t per PE through execute(), on two pinned buffers
// the library allocates once (State::collect_lens).  Then every PE builds PLAN_COLLECT
// from the same P lengths.
void exchange_lengths(const Team &t, uint64_t mine, uint64_t *lens, const char *fn)
{
    uint64_t *&buf = st().collect_lens;  // [0]: this PE's length; [1, 1 + PLAN_MAX_PE): everyone's
    if (!buf)
        hip_check(hipHostMalloc((void **)&buf, (1 + sosplan::PLAN_MAX_PE) * sizeof(uint64_t), hipHostMallocDefault),
                  "hipHostMalloc(collect lengths)");
    buf[0] = mine;
    execute(sosplan::PLAN_FCOLLECT, buf + 1, buf, 1, sizeof(uint64_t), t, SOSX_OP_SUM, SOSX_DT_UCHAR, fn);
    memcpy(lens, buf + 1, (size_t)t.size * sizeof(uint64_t));
}

// The checked part shared by the team and active-set forms, in SOS's order
// (src/collectives_c.c4:436-441, :468-473).  One deviation: once the
// lengths are known, the target's TRUE extent -- the sum of the lengths -- is checked for
// symmetry and for overlap with the source; SOS has written by the time it could know.
void collect_checked(const Team &t, void *dest, const void *source, size_t nelems, size_t es,
                     const long *pSync, const char *fn)
{
    const size_t sb = checked_bytes(nelems, es, "nelems", fn);
    check_symmetric(dest, sb, "dest", fn);
    check_symmetric(source, sb, "source", fn);
    if (pSync) check_symmetric(pSync, sizeof(long) * SHMEM_COLLECT_SYNC_SIZE, "pSync", fn);
    check_overlap2(dest, sb, source, sb, fn);
    check_member(t, fn);
    if (t.size == 1) {  // src/collectives.c:1229-1232
        if (sb) local_copy(dest, source, sb, fn);
        return;
    }
    check_team_size(t, fn);
    // nelems == 0 is legal and that PE still takes part: its peers need its length
    uint64_t lens[sosplan::PLAN_MAX_PE];
    bool all_payload = false;
    const bool slots = small_collect_exchange(t, source, sb, lens, &all_payload, fn);
    if (!slots) exchange_lengths(t, sb, lens, fn);
    uint64_t sum = 0;
    for (int q = 0; q < t.size; ++q) {
        if (lens[q] > (uint64_t)SIZE_MAX - sum)
            raise_error("%s: the contributions of the %d PEs overflow size_t", fn, t.size);
        sum += lens[q];
    }
    if (sum) {
        check_symmetric(dest, (size_t)sum, "dest", fn);
        check_overlap2(dest, (size_t)sum, source, sb, fn);
    }
    // every payload attached (a uniform fact of the headers): one kernel writes the target
    if (slots) small_collect_finish(t, dest, lens, all_payload, fn);
    if (sum == 0 || (slots && all_payload)) return;  // every PE sees the same lengths
    execute(sosplan::PLAN_COLLECT, dest, source, 0, 1, t, SOSX_OP_SUM, SOSX_DT_UCHAR, fn, false, lens);
}

// alltoalls is PLAN_ALLTOALL over packed operands.  The block for peer j starts at
// source + j*nelems*sst*es with elements sst apart (src/collectives.c:1514-1521) and the
// block from PE i lands at dest + i*nelems*dst*es (:1489): the whole source is ONE strided
// run of P*nelems elements, and so is the whole target.  A strided operand is packed
// (source) or unpacked (target) by sosx_strided_copy when it is device memory and by a
// host loop when it is host memory (a kernel cannot reach pageable memory); an operand
// at stride 1 goes to the executor as it is and runs in place where the executor allows.
// The unpack writes elements only, into the caller's target: the gaps keep their bytes.
void alltoalls_checked(const Team &t, void *dest, const void *source, ptrdiff_t dst, ptrdiff_t sst,
                       size_t nelems, size_t es, const long *pSync, const char *fn)
{
    State &s = st();
    const size_t N = checked_bytes(nelems, (size_t)t.size, "nelems", fn);
    const size_t bytes = checked_bytes(N, es, "nelems", fn);
    if (N) {
        check_symmetric(dest, strided_extent(N, dst, es, fn), "dest", fn);
        check_symmetric(source, strided_extent(N, sst, es, fn), "source", fn);
    }
    if (pSync) check_symmetric(pSync, sizeof(long) * SHMEM_ALLTOALLS_SYNC_SIZE, "pSync", fn);
    check_member(t, fn);
    if (nelems == 0) return;  // src/collectives.c:1494
    check_team_size(t, fn);
    const bool dev_s = is_device_ptr(source), dev_d = is_device_ptr(dest);
    const size_t slot = align256(bytes);
    // device slots for the packed operands: the exchange scratch, which the alltoall
    // plan itself never uses
    char *wk = nullptr;
    if ((sst != 1 && dev_s) || (dst != 1 && dev_d)) wk = (char *)scratch(2 * slot);
    std::vector<char> hsrc, hdst;
    const void *psrc = source;
    if (sst != 1 && dev_s) {
        int rc = sosx_strided_copy(wk, 1, source, sst, es, N, s.stream);
        if (rc) raise_error("%s: %s", fn, status_text(rc));
        psrc = wk;
    } else if (sst != 1) {
        hsrc.resize(bytes);
        const char *sp = (const char *)source;
        for (size_t k = 0; k < N; ++k) memcpy(&hsrc[k * es], sp + k * (size_t)sst * es, es);
        psrc = hsrc.data();
    }
    const void *packed = psrc;  // where the packed result is (team of one: the packed source)
    if (t.size > 1) {
        void *pdst = dest;
        if (dst != 1 && dev_d) pdst = wk + slot;
        else if (dst != 1) {
            hdst.resize(bytes);
            pdst = hdst.data();
        }
        execute(sosplan::PLAN_ALLTOALL, pdst, psrc, nelems, es, t, SOSX_OP_SUM, SOSX_DT_UCHAR, fn);
        packed = pdst;
    }
    if (dst == 1) {
        if (t.size == 1) local_copy(dest, packed, bytes, fn);
        else if (psrc == wk) hip_check(sync_system(s.stream), fn);
        return;
    }
    if (dev_d) {
        if (!is_device_ptr(packed)) {  // team of one, host source
            hip_check(hipMemcpyAsync(wk + slot, packed, bytes, hipMemcpyHostToDevice, s.stream), fn);
            packed = wk + slot;
        }
        int rc = sosx_strided_copy(dest, dst, packed, 1, es, N, s.stream);
        if (rc) raise_error("%s: %s", fn, status_text(rc));
        hip_check(sync_system(s.stream), fn);
        return;
    }
    if (is_device_ptr(packed)) {  // team of one, device source
        hdst.resize(bytes);
        hip_check(hipMemcpyAsync(hdst.data(), packed, bytes, hipMemcpyDeviceToHost, s.stream), fn);
        hip_check(sync_system(s.stream), fn);
        packed = hdst.data();
    }
    char *dp = (char *)dest;
    for (size_t k = 0; k < N; ++k) memcpy(dp + k * (size_t)dst * es, (const char *)packed + k * es, es);
}

}  // namespace
}  // extern "C"

// ---- reductions, broadcasts, scans -------------------------------------------------------
namespace {

// Small operands (host-resident, or device-resident below SHMEMX_SMALL_DEVICE) go through
// the node shared segment: one kernel per PE reading every PE's operand in place
// (smallpath.cpp), no DMA copies; everything else runs its plan on the executors.  The
// route is published and checked on every call of a team of two or more (`allowed`: the
// call may take the small path at all); a team of one has nobody to agree with.
void route_or_execute(int plan, void *target, const void *source, size_t count, size_t ts,
                      const Team &t, int op, int dt, const char *fn, bool allowed = true,
                      bool reduction = false)
{
    if (t.size > 1 && small_path_route(plan, target, source, count * ts, t, allowed, fn))
        small_path_reduce(plan, target, source, count, ts, t, op, dt, fn);
    else
        execute(plan, target, source, count, ts, t, op, dt, fn, reduction);
}

// shmem_internal_op_to_all for this PE over team t.
void op_to_all(void *target, const void *source, size_t count, size_t ts, const Team &t, int op,
               int dt, const char *fn)
{
    State &s = st();
    if (count == 0) return;
    const size_t bytes = count * ts;
    // PE_size 1: copy (src/collectives.c:664-668), no combine, any datatype
    if (t.size == 1) return local_copy(target, source, bytes, fn);
    int rc = sos_check_op(op, dt);
    if (rc) raise_error("%s: %s (datatype %d, op %d)", fn, status_text(rc), dt, op);

    int alg = sosplan::resolve_alg(s.reduce_alg, bytes, s.coll_size_crossover);
    // the one-kernel forms fold at most SOSX_MAX_FOLD inputs: bigger teams keep the
    // same element order through the pairwise schedules (ring/recdbl_direct: recdbl_sw
    // tree by recursive halving; recdbl_gather: recdbl_sw itself)
    if ((alg == SOSX_ALG_RING || alg == SOSX_ALG_RECDBL_DIRECT) && t.size > SOSX_MAX_FOLD)
        alg = SOSX_ALG_RECHALVING;
    if (alg == SOSX_ALG_RECDBL_GATHER && sosplan::pow2_floor(t.size) > SOSX_MAX_FOLD)
        alg = SOSX_ALG_RECDBL;
    // the small path for recdbl_sw below the crossover and the ring above it, unless
    // SHMEMX_RCCL_ALLREDUCE hands reductions to RCCL
    route_or_execute(alg, target, source, count, ts, t, op, dt, fn, !s.rccl_allreduce, true);
}

void bcast_active_set(void *target, const void *source, size_t nlong, size_t ts, int PE_root,
                      int PE_start, int logPE_stride, int PE_size, long *pSync, const char *fn)
{
    check_initialized(fn);
    const Team t = active_set_team(PE_start, logPE_stride, PE_size, fn);
    check_root(PE_root, PE_size, fn);
    const size_t bytes = checked_bytes(nlong, ts, "nlong", fn);
    check_symmetric(target, bytes, "target", fn);
    check_symmetric(source, bytes, "source", fn);
    check_symmetric(pSync, sizeof(long) * SHMEM_BCAST_SYNC_SIZE, "pSync", fn);
    check_overlap(target, source, bytes, fn);
    if (PE_size == 1 || bytes == 0) return;  // src/collectives.c:441
    // the root's target is not written (collectives_c.c4:342-378)
    route_or_execute(sosplan::bcast_alg(PE_root, false), target, source, nlong, ts, t, SOSX_OP_SUM,
                     SOSX_DT_UCHAR, fn);
}

}  // namespace

extern "C" {

void sos_api_to_all(void *target, const void *source, int nreduce, size_t type_size,
                    int PE_start, int logPE_stride, int PE_size, void *pWrk, long *pSync, int op,
                    int datatype, const char *fn)
{
    check_initialized(fn);
    const Team t = active_set_team(PE_start, logPE_stride, PE_size, fn);
    if (nreduce < 0)
        raise_error("%s: Argument nreduce must be greater or equal to zero (%ld)", fn, (long)nreduce);
    const size_t bytes = (size_t)nreduce * type_size;
    check_symmetric(target, bytes, "target", fn);
    check_symmetric(source, bytes, "source", fn);
    const size_t wrk = (size_t)(nreduce / 2 + 1 > SHMEM_REDUCE_MIN_WRKDATA_SIZE
                                    ? nreduce / 2 + 1 : SHMEM_REDUCE_MIN_WRKDATA_SIZE);
    check_symmetric(pWrk, type_size * wrk, "pWrk", fn);
    check_symmetric(pSync, sizeof(long) * SHMEM_REDUCE_SYNC_SIZE, "pSync", fn);
    check_overlap(target, source, bytes, fn);
    // pWrk is never touched by any SOS reduction algorithm; pSync holds
    // SHMEM_SYNC_VALUE on entry and is left so (RCCL does the synchronisation).
    op_to_all(target, source, (size_t)nreduce, type_size, t, op, datatype, fn);
}

int sos_api_reduce(shmem_team_t team, void *dest, const void *source, size_t nreduce,
                   size_t type_size, int op, int datatype, const char *fn)
{
    check_initialized(fn);
    const Team *t = checked_team(team, fn);
    const size_t bytes = checked_bytes(nreduce, type_size, "nreduce", fn);
    check_symmetric(dest, bytes, "dest", fn);
    check_symmetric(source, bytes, "source", fn);
    check_overlap(dest, source, bytes, fn);
    check_member(*t, fn);
    op_to_all(dest, source, nreduce, type_size, *t, op, datatype, fn);
    return 0;
}

int sos_api_broadcast(shmem_team_t team, void *dest, const void *source, size_t nelems,
                      size_t type_size, int PE_root, const char *fn)
{
    check_initialized(fn);
    const Team *t = checked_team(team, fn);
    const size_t bytes = checked_bytes(nelems, type_size, "nelems", fn);
    check_symmetric(dest, bytes, "dest", fn);
    check_symmetric(source, bytes, "source", fn);
    check_overlap(dest, source, bytes, fn);
    check_member(*t, fn);
    check_root(PE_root, t->size, fn);
    if (bytes == 0) return 0;
    // the team forms copy source to dest on the root as well (collectives_c.c4:390-397)
    route_or_execute(sosplan::bcast_alg(PE_root, true), dest, source, nelems, type_size, *t,
                     SOSX_OP_SUM, SOSX_DT_UCHAR, fn);
    return 0;
}

void pshmem_broadcast32(void *target, const void *source, size_t nlong, int PE_root, int PE_start,
                        int logPE_stride, int PE_size, long *pSync)
{
    bcast_active_set(target, source, nlong, 4, PE_root, PE_start, logPE_stride, PE_size, pSync,
                     "shmem_broadcast32");
}

void pshmem_broadcast64(void *target, const void *source, size_t nlong, int PE_root, int PE_start,
                        int logPE_stride, int PE_size, long *pSync)
{
    bcast_active_set(target, source, nlong, 8, PE_root, PE_start, logPE_stride, PE_size, pSync,
                     "shmem_broadcast64");
}

int pshmem_broadcastmem(shmem_team_t team, void *dest, const void *source, size_t nelems,
                        int PE_root)
{
    return sos_api_broadcast(team, dest, source, nelems, 1, PE_root, "shmem_broadcastmem");
}

void shmem_broadcast32(void *, const void *, size_t, int, int, int, int, long *)
    __attribute__((weak, alias("pshmem_broadcast32")));
void shmem_broadcast64(void *, const void *, size_t, int, int, int, int, long *)
    __attribute__((weak, alias("pshmem_broadcast64")));
int shmem_broadcastmem(shmem_team_t, void *, const void *, size_t, int)
    __attribute__((weak, alias("pshmem_broadcastmem")));

int sos_api_scan(shmem_team_t team, void *dest, const void *source, size_t nelems,
                 size_t type_size, int op, int datatype, int exclusive, const char *fn)
{
    check_initialized(fn);
    const Team *t = checked_team(team, fn);
    const size_t bytes = checked_bytes(nelems, type_size, "nelems", fn);
    check_symmetric(dest, bytes, "dest", fn);
    check_symmetric(source, bytes, "source", fn);
    check_overlap(dest, source, bytes, fn);
    check_member(*t, fn);
    if (nelems == 0) return 0;
    int rc = sos_check_op(op, datatype);
    if (rc) raise_error("%s: %s (datatype %d, op %d)", fn, status_text(rc), datatype, op);
    check_team_size(*t, fn);
    route_or_execute(exclusive ? sosplan::PLAN_EXSCAN : sosplan::PLAN_INSCAN, dest, source, nelems,
                     type_size, *t, op, datatype, fn);
    return 0;
}

int sos_api_fcollect(shmem_team_t team, void *dest, const void *source, size_t nelems,
                     size_t type_size, const char *fn)
{
    check_initialized(fn);
    fcollect_checked(*checked_team(team, fn), dest, source, nelems, type_size, nullptr, fn);
    return 0;
}

int sos_api_collect(shmem_team_t team, void *dest, const void *source, size_t nelems,
                    size_t type_size, const char *fn)
{
    check_initialized(fn);
    collect_checked(*checked_team(team, fn), dest, source, nelems, type_size, nullptr, fn);
    return 0;
}

void sos_api_collect_active(void *target, const void *source, size_t nlong, size_t type_size,
                            int PE_start, int logPE_stride, int PE_size, long *pSync, const char *fn)
{
    check_initialized(fn);
    const Team t = active_set_team(PE_start, logPE_stride, PE_size, fn);
    // pSync is only checked: it holds SHMEM_SYNC_VALUE on entry and is left so
    collect_checked(t, target, source, nlong, type_size, pSync, fn);
}

int sos_api_alltoall(shmem_team_t team, void *dest, const void *source, size_t nelems,
                     size_t type_size, const char *fn)
{
    check_initialized(fn);
    alltoall_checked(*checked_team(team, fn), dest, source, nelems, type_size, nullptr, fn);
    return 0;
}

int sos_api_alltoalls(shmem_team_t team, void *dest, const void *source, ptrdiff_t dst,
                      ptrdiff_t sst, size_t nelems, size_t type_size, const char *fn)
{
    check_initialized(fn);
    check_positive(sst, "sst", fn);
    check_positive(dst, "dst", fn);
    alltoalls_checked(*checked_team(team, fn), dest, source, dst, sst, nelems, type_size, nullptr, fn);
    return 0;
}

int pshmem_fcollectmem(shmem_team_t team, void *dest, const void *source, size_t nelems)
{
    return sos_api_fcollect(team, dest, source, nelems, 1, "shmem_fcollectmem");
}

int pshmem_alltoallmem(shmem_team_t team, void *dest, const void *source, size_t nelems)
{
    return sos_api_alltoall(team, dest, source, nelems, 1, "shmem_alltoallmem");
}

int pshmem_alltoallsmem(shmem_team_t team, void *dest, const void *source, ptrdiff_t dst,
                        ptrdiff_t sst, size_t nelems)
{
    return sos_api_alltoalls(team, dest, source, dst, sst, nelems, 1, "shmem_alltoallsmem");
}

#define SOS_DEF_ACTIVE_SET_COLLECTS(BITS, ES)                                                      \
    void pshmem_fcollect##BITS(void *target, const void *source, size_t nlong, int PE_start,       \
                               int logPE_stride, int PE_size, long *pSync)                         \
    {                                                                                              \
        const char *fn = "shmem_fcollect" #BITS;                                                   \
        check_initialized(fn);                                                                     \
        const Team t = active_set_team(PE_start, logPE_stride, PE_size, fn);                       \
        fcollect_checked(t, target, source, nlong, ES, pSync, fn);                                 \
    }                                                                                              \
    void pshmem_alltoall##BITS(void *dest, const void *source, size_t nelems, int PE_start,        \
                               int logPE_stride, int PE_size, long *pSync)                         \
    {                                                                                              \
        const char *fn = "shmem_alltoall" #BITS;                                                   \
        check_initialized(fn);                                                                     \
        const Team t = active_set_team(PE_start, logPE_stride, PE_size, fn);                       \
        alltoall_checked(t, dest, source, nelems, ES, pSync, fn);                                  \
    }                                                                                              \
    void pshmem_alltoalls##BITS(void *dest, const void *source, ptrdiff_t dst, ptrdiff_t sst,      \
                                size_t nelems, int PE_start, int logPE_stride, int PE_size,        \
                                long *pSync)                                                       \
    {                                                                                              \
        const char *fn = "shmem_alltoalls" #BITS;                                                  \
        check_initialized(fn);                                                                     \
        check_positive(sst, "sst", fn);                                                            \
        check_positive(dst, "dst", fn);                                                            \
        const Team t = active_set_team(PE_start, logPE_stride, PE_size, fn);                       \
        alltoalls_checked(t, dest, source, dst, sst, nelems, ES, pSync, fn);                       \
    }                                                                                              \
    void shmem_fcollect##BITS(void *, const void *, size_t, int, int, int, long *)                 \
        __attribute__((weak, alias("pshmem_fcollect" #BITS)));                                     \
    void shmem_alltoall##BITS(void *, const void *, size_t, int, int, int, long *)                 \
        __attribute__((weak, alias("pshmem_alltoall" #BITS)));                                     \
    void shmem_alltoalls##BITS(void *, const void *, ptrdiff_t, ptrdiff_t, size_t, int, int, int,  \
                               long *) __attribute__((weak, alias("pshmem_alltoalls" #BITS)));

SOS_DEF_ACTIVE_SET_COLLECTS(32, 4)
SOS_DEF_ACTIVE_SET_COLLECTS(64, 8)

int shmem_fcollectmem(shmem_team_t, void *, const void *, size_t)
    __attribute__((weak, alias("pshmem_fcollectmem")));
int shmem_alltoallmem(shmem_team_t, void *, const void *, size_t)
    __attribute__((weak, alias("pshmem_alltoallmem")));
int shmem_alltoallsmem(shmem_team_t, void *, const void *, ptrdiff_t, ptrdiff_t, size_t)
    __attribute__((weak, alias("pshmem_alltoallsmem")));

int shmemx_reduce_local(int op, int datatype, size_t count, const void *in, void *inout)
{
    check_initialized("shmemx_reduce_local");
    // One completion rule for every residency, as SOS's CPU loop: the result is in
    // `inout` when the call returns.
    int rc = sos_check_op(op, datatype);
    if (rc || count == 0) return rc;
    if (!inout || !in) return SOSX_ERR_ARG;
    const bool dev_io = is_device_ptr(inout), dev_in = is_device_ptr(in);
    // small operands, same residency: one launch, completion words (smallpath.cpp)
    if (small_local_combine(op, datatype, inout, in, count, sosx_dtype_size(datatype), dev_io, dev_in))
        return SOSX_OK;
    // both on the host (the SOS heap): H2D || combine || D2H pipeline, synchronous
    if (!dev_io && !dev_in) return sosx_combine_host(op, datatype, inout, in, count, 0);
    State &s = st();
    if (dev_io && dev_in) {
        rc = sosx_combine(op, datatype, inout, in, count, s.stream);
    } else {
        // mixed residency: the kernel never dereferences host memory; the host operand
        // is staged through HBM (and `inout` copied back when it is the host one)
        const size_t bytes = count * sosx_dtype_size(datatype);
        void *d = stage(bytes);
        if (hipMemcpyAsync(d, dev_io ? in : inout, bytes, hipMemcpyHostToDevice, s.stream) !=
            hipSuccess)
            return SOSX_ERR_HIP;
        rc = dev_io ? sosx_combine(op, datatype, inout, d, count, s.stream)
                    : sosx_combine(op, datatype, d, in, count, s.stream);
        if (!rc && !dev_io &&
            hipMemcpyAsync(inout, d, bytes, hipMemcpyDeviceToHost, s.stream) != hipSuccess)
            return SOSX_ERR_HIP;
    }
    if (rc) return rc;
    return sync_system(s.stream) == hipSuccess ? SOSX_OK : SOSX_ERR_HIP;
}

}  // extern "C"
