// sync_eval_harness.cpp -- a program of its own (no HIP, no Python) over the host-only
// part of put-with-signal and the point-to-point waits (sos_amd/csrc/onesided_checks.cpp,
// compiled into it): sos_sync_eval against a model written from SOS's loops
// (src/synchronization_c.c4), sos_put_signal_check and sos_sync_check over hand-built
// layouts, and the copy split of sosx_put_signal (putsignal_plan.h) walked as the kernel's
// workgroups walk it.  Buffers have the exact extents, so AddressSanitizer sees an access
// one byte out.  Built plain and with -fsanitize=address,undefined by
// tests/test_sync_eval_harness.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "api_internal.h"
#include "putsignal_plan.h"

static long g_cases = 0, g_bad = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        ++g_cases;                        \
        if (!(cond)) {                    \
            if (++g_bad <= 10) {          \
                fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);                        \
                fprintf(stderr, "\n");    \
            }                             \
        }                                 \
    } while (0)

// ---- the model: SHMEM_TEST at the type's own width and sign ---------------------------------
template <class T> static bool model_cmp(int cmp, T a, T b)
{
    switch (cmp) {
        case 1: return a == b;
        case 2: return a != b;
        case 3: return a > b;
        case 4: return a >= b;
        case 5: return a < b;
        default: return a <= b;
    }
}

template <class T> static void sweep_eval(int is_signed)
{
    const T lo = is_signed ? (T)((uint64_t)1 << (8 * sizeof(T) - 1)) : (T)0;
    const T hi = is_signed ? (T)~lo : (T)~(T)0;
    const T pool[] = {(T)0, (T)1, (T)-1, lo, hi, (T)(lo + 1), (T)(hi - 1), (T)42};
    const size_t npool = sizeof(pool) / sizeof(pool[0]);
    for (size_t nelems : {(size_t)0, (size_t)1, (size_t)3, (size_t)65}) {
        // exact extents: a read past nelems words is out of bounds
        std::vector<T> words(nelems), values(nelems ? nelems : 1);
        std::vector<int> status(nelems);
        std::vector<size_t> indices(nelems), want_idx;
        for (int mask = 0; mask < 4; ++mask)       // none (NULL), none (zeros), partly, all
            for (int cmp = 1; cmp <= 6; ++cmp)
                for (size_t rot = 0; rot < npool; ++rot)
                    for (int vector = 0; vector < 2; ++vector) {
                        for (size_t i = 0; i < nelems; ++i) {
                            words[i] = pool[(i + rot) % npool];
                            values[i] = pool[(i * 3 + rot + 1) % npool];
                            status[i] = mask == 3 ? 1 : mask == 2 ? (int)((i + rot) % 3 == 0) : 0;
                        }
                        values[0] = pool[(rot + 1) % npool];
                        const int *st = mask == 0 ? nullptr : status.data();
                        size_t live = 0, hold = 0, first = SIZE_MAX;
                        want_idx.clear();
                        for (size_t i = 0; i < nelems; ++i) {
                            if (st && st[i]) continue;
                            ++live;
                            if (model_cmp<T>(cmp, words[i], values[vector ? i : 0])) {
                                if (first == SIZE_MAX) first = i;
                                want_idx.push_back(i);
                                ++hold;
                            }
                        }
                        for (int kind = SOS_SYNC_ONE; kind <= SOS_SYNC_SOME; ++kind) {
                            if (kind == SOS_SYNC_ONE && (nelems != 1 || st)) continue;
                            size_t index = 77, count = 77;
                            std::fill(indices.begin(), indices.end(), (size_t)99);
                            const int r = sos_sync_eval(nelems ? words.data() : nullptr, nelems, sizeof(T), is_signed, st, cmp,
                                                        values.data(), vector, kind, &index, nelems ? indices.data() : nullptr,
                                                        &count);
                            int want;
                            if (!live) want = 1;
                            else if (kind == SOS_SYNC_ONE || kind == SOS_SYNC_ALL) want = hold == live;
                            else want = hold > 0;
                            CHECK(r == want, "eval width %zu signed %d n %zu mask %d cmp %d kind %d vector %d: %d, want %d",
                                  sizeof(T), is_signed, nelems, mask, cmp, kind, vector, r, want);
                            CHECK(index == (kind == SOS_SYNC_ANY ? first : SIZE_MAX), "any index %zu, want %zu", index, first);
                            CHECK(count == (kind == SOS_SYNC_SOME ? hold : 0), "some count %zu, want %zu", count, hold);
                            if (kind == SOS_SYNC_SOME)
                                for (size_t k = 0; k < nelems; ++k)
                                    CHECK(indices[k] == (k < hold ? want_idx[k] : 99), "some indices[%zu] = %zu", k, indices[k]);
                        }
                    }
    }
}

// ---- the checks over a made-up layout ------------------------------------------------------------
static const uintptr_t DEV = 0x7F0000000000, HOSTH = 0x500000000000, DATA = 0x600000, LOCAL = 0x10000;
static const size_t DEV_SIZE = 1 << 20, HOSTH_SIZE = 1 << 16, DATA_SIZE = 4096;

static int put_check(sos_put_signal_op op, int initialized = 1, int my_pe = 1, int mapped = 1, char *msg = nullptr)
{
    const sos_rma_region regions[3] = {{DEV, DEV_SIZE, SOS_RMA_REGION_DEVICE_HEAP},
                                       {HOSTH, HOSTH_SIZE, SOS_RMA_REGION_HOST_HEAP},
                                       {DATA, DATA_SIZE, SOS_RMA_REGION_DATA}};
    const sos_rma_layout lay = {initialized, my_pe, 4, mapped, 3, regions};
    char buf[512];
    return sos_put_signal_check(&lay, &op, msg ? msg : buf, 512);
}

static int sync_check(sos_sync_op op, int initialized = 1, char *msg = nullptr)
{
    const sos_rma_region regions[2] = {{DEV, DEV_SIZE, SOS_RMA_REGION_DEVICE_HEAP},
                                       {HOSTH, HOSTH_SIZE, SOS_RMA_REGION_HOST_HEAP}};
    const sos_rma_layout lay = {initialized, 1, 4, 1, 2, regions};
    char buf[512];
    return sos_sync_check(&lay, &op, msg ? msg : buf, 512);
}

static const void *P(uintptr_t v) { return (const void *)v; }

static void sweep_checks()
{
    // sos_put_signal_op: target, source, sig_addr, nelems, type_size, sig_op, pe
    const sos_put_signal_op good = {P(DEV + 64), P(LOCAL), P(DEV + 4096), 8, 8, 0, 2};
    CHECK(put_check(good) == SOS_RMA_OK, "a plain put_signal is accepted");
    sos_put_signal_op op = good;
    CHECK(put_check(op, 0) == SOS_RMA_NOT_INITIALIZED, "not initialized");
    op.pe = 4;
    CHECK(put_check(op) == SOS_RMA_BAD_PE, "PE 4 of 4");
    op.target = P(LOCAL);                           // two defects: the PE comes first
    CHECK(put_check(op) == SOS_RMA_BAD_PE, "PE before symmetric");
    op = good;
    op.target = P(DEV + DEV_SIZE - 32);
    CHECK(put_check(op) == SOS_RMA_NOT_SYMMETRIC, "target runs over the heap's end");
    op.nelems = 4;
    CHECK(put_check(op) == SOS_RMA_OK, "the heap's last bytes");
    op = good;
    op.source = nullptr;
    CHECK(put_check(op) == SOS_RMA_NULL_LOCAL, "NULL source");
    op.nelems = 0;
    CHECK(put_check(op) == SOS_RMA_OK, "NULL source with nothing to move");
    op = good;
    op.pe = 1;
    op.sig_addr = P(DEV + 64 + 56);
    CHECK(put_check(op) == SOS_RMA_OVERLAP, "sig_addr inside the target, to the PE itself");
    op.pe = 2;
    CHECK(put_check(op) == SOS_RMA_OK, "the overlap check is for pe == my_pe only, as SOS's");
    op = good;
    op.sig_op = 2;
    CHECK(put_check(op) == SOS_SIG_BAD_OP, "sig_op 2");
    op.sig_addr = P(LOCAL);                         // two defects: SOS's sig_op check comes first
    CHECK(put_check(op) == SOS_SIG_BAD_OP, "sig_op before this library's sig_addr checks");
    op.sig_op = 1;
    CHECK(put_check(op) == SOS_RMA_NOT_SYMMETRIC, "sig_addr not symmetric");
    op.sig_addr = P(DEV + 4100);
    CHECK(put_check(op) == SOS_RMA_BAD_TYPE_SIZE, "sig_addr not 8-byte aligned");
    op = good;
    op.sig_addr = P(HOSTH + 8);
    CHECK(put_check(op) == SOS_RMA_PEER_NOT_DEVICE_HEAP, "a peer's signal in the host heap");
    op.pe = 1;
    CHECK(put_check(op, 1, 1, 0) == SOS_RMA_OK, "the PE itself: any symmetric memory, no mapping");
    op = good;
    CHECK(put_check(op, 1, 1, 0) == SOS_RMA_NO_PATH, "peer heap not mapped");
    for (uintptr_t region : {DEV, HOSTH, DATA}) {
        op = {P(region + 64), P(LOCAL), P(region + 1024), 4, 4, 1, 1};
        CHECK(put_check(op) == SOS_RMA_OK, "self-PE put_signal in region %#lx", (unsigned long)region);
    }
    // sos_sync_op: ivars, nelems, type_size, status, indices, kind, cmp
    const sos_sync_op sgood = {P(DEV + 64), 4, 8, P(LOCAL), P(LOCAL + 64), SOS_SYNC_SOME, 4};
    CHECK(sync_check(sgood) == SOS_RMA_OK, "a plain wait_until_some is accepted");
    sos_sync_op s = sgood;
    CHECK(sync_check(s, 0) == SOS_RMA_NOT_INITIALIZED, "not initialized");
    s.ivars = P(LOCAL + 4096);
    s.cmp = 9;                                      // two defects: symmetric first
    CHECK(sync_check(s) == SOS_RMA_NOT_SYMMETRIC, "ivars not symmetric, before the comparison");
    s = sgood;
    s.ivars = P(DEV + DEV_SIZE - 16);
    CHECK(sync_check(s) == SOS_RMA_NOT_SYMMETRIC, "ivars run over the heap's end");
    s = sgood;
    s.indices = P(LOCAL + 8);
    CHECK(sync_check(s) == SOS_RMA_OVERLAP, "indices overlap status");
    s = sgood;
    s.status = P(DEV + 64 + 16);
    CHECK(sync_check(s) == SOS_RMA_OVERLAP, "status inside the ivars");
    s = sgood;
    s.indices = P(DEV + 64 - 8);
    CHECK(sync_check(s) == SOS_RMA_OVERLAP, "indices run into the ivars");
    s = sgood;
    s.status = nullptr;
    CHECK(sync_check(s) == SOS_RMA_OK, "status NULL");
    for (int cmp : {0, 7, -1}) {
        s = sgood;
        s.cmp = cmp;
        CHECK(sync_check(s) == SOS_SYNC_BAD_CMP, "comparison %d", cmp);
    }
    s = sgood;
    s.ivars = P(DEV + 68);
    CHECK(sync_check(s) == SOS_RMA_BAD_TYPE_SIZE, "ivars not aligned to their size");
    s.type_size = 4;
    CHECK(sync_check(s) == SOS_RMA_OK, "4-byte ivars at a 4-byte offset");
    s.type_size = 2;
    s.ivars = P(HOSTH + 2);
    s.kind = SOS_SYNC_ONE;
    s.nelems = 1;
    CHECK(sync_check(s) == SOS_RMA_OK, "a short in the host heap at a 2-byte offset");
    s.type_size = 1;
    CHECK(sync_check(s) == SOS_RMA_BAD_TYPE_SIZE, "1-byte ivars");
}

// ---- the copy split of sosx_put_signal, walked as the kernel walks it ------------------------------
static void sweep_plan()
{
    using namespace sos;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)8, (size_t)15, (size_t)16, (size_t)17, (size_t)61, (size_t)4095,
                     (size_t)4096, (size_t)4097, (size_t)8207, (size_t)8208, (size_t)70001})
        for (unsigned dmis = 0; dmis < 16; ++dmis)
            for (unsigned smis = 0; smis < 16; ++smis) {
                // exact extents behind 16-B aligned bases
                std::vector<unsigned char> sbuf(16 + smis + n), dbuf(16 + dmis + n);
                unsigned char *s = sbuf.data() + (16 - (uintptr_t)sbuf.data() % 16) % 16 + smis;
                unsigned char *d = dbuf.data() + (16 - (uintptr_t)dbuf.data() % 16) % 16 + dmis;
                if (s + n > sbuf.data() + sbuf.size() || d + n > dbuf.data() + dbuf.size()) continue;
                for (size_t i = 0; i < n; ++i) s[i] = (unsigned char)(i * 31 + smis);
                std::vector<unsigned char> written(n, 0);
                const PsPlan p = ps_plan((uintptr_t)d, (uintptr_t)s, n);
                bool ok = p.head + p.units * p.width + p.tail == n && p.grid >= 1 && p.grid <= kPsMaxGrid &&
                          p.head + p.tail < kPsThreads;
                for (unsigned wg = 0; wg < p.grid && ok; ++wg) {
                    for (uint64_t t = wg; t < p.tiles; t += p.grid)
                        for (uint64_t u = t * kPsTile; u < (t + 1) * kPsTile && u < p.units; ++u) {
                            const uint64_t off = p.head + u * p.width;
                            ok = ok && ((uintptr_t)(d + off) % p.width == 0);
                            ok = ok && ((uintptr_t)(s + off) % (p.unaligned_loads ? 4 : p.width) == 0);
                            memcpy(d + off, s + off, p.width);
                            for (unsigned b = 0; b < p.width; ++b) ++written[off + b];
                        }
                    if (wg == 0)
                        for (uint64_t k = 0; k < p.head + p.tail; ++k) {
                            const uint64_t off = k < p.head ? k : p.head + p.units * p.width + (k - p.head);
                            d[off] = s[off];
                            ++written[off];
                        }
                }
                for (size_t i = 0; i < n && ok; ++i) ok = written[i] == 1 && d[i] == s[i];
                CHECK(ok, "put_signal plan n %zu dmis %u smis %u: width %u ul %d head %llu units %llu tail %llu grid %u", n,
                      dmis, smis, p.width, p.unaligned_loads, (unsigned long long)p.head, (unsigned long long)p.units,
                      (unsigned long long)p.tail, p.grid);
            }
}

int main()
{
    sweep_eval<int16_t>(1);
    sweep_eval<uint16_t>(0);
    sweep_eval<int32_t>(1);
    sweep_eval<uint32_t>(0);
    sweep_eval<int64_t>(1);
    sweep_eval<uint64_t>(0);
    // a short of -1 is not 65535
    const int16_t m1 = -1, zero = 0;
    size_t idx, cnt;
    CHECK(sos_sync_eval(&m1, 1, 2, 1, nullptr, 5, &zero, 0, SOS_SYNC_ONE, &idx, nullptr, &cnt) == 1, "short -1 < 0");
    CHECK(sos_sync_eval(&m1, 1, 2, 0, nullptr, 5, &zero, 0, SOS_SYNC_ONE, &idx, nullptr, &cnt) == 0, "ushort 65535 < 0");
    CHECK(sos_sync_eval(&m1, 1, 3, 1, nullptr, 5, &zero, 0, SOS_SYNC_ONE, &idx, nullptr, &cnt) == -1, "width 3");
    CHECK(sos_sync_eval(&m1, 1, 2, 1, nullptr, 0, &zero, 0, SOS_SYNC_ONE, &idx, nullptr, &cnt) == -1, "comparison 0");
    sweep_checks();
    sweep_plan();
    if (g_bad) {
        fprintf(stderr, "%ld of %ld cases FAILED\n", g_bad, g_cases);
        return 1;
    }
    printf("sync eval, checks and put_signal plans OK: %ld cases\n", g_cases);
    return 0;
}
