// onesided_checks_harness.cpp -- a program of its own over the layout-based argument checks
// of the one-sided layer (sos_amd/csrc/onesided_checks.cpp, compiled next to it; no HIP, no
// library): sos_rma_check, sos_amo_check, sos_put_signal_check and sos_lock_check over a
// made-up layout, each case asked four ways -- with a 512-byte message buffer, with
// msg == NULL, with n == 0 and with a buffer of exactly one byte from the heap.  The code
// must be the same every time, the one-byte buffer must end up an empty string, and the
// buffer that may not be written must keep its canary.  Built plain and with the address and
// undefined-behaviour sanitizers (tests/test_onesided_refusals.py): a message written past
// its buffer, or an address of the layout dereferenced, would be reported there.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#include "onesided_checks.h"

static int checks = 0, failed = 0;

#define EXPECT(cond)                                                   \
    do {                                                               \
        ++checks;                                                      \
        if (!(cond)) {                                                 \
            ++failed;                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                              \
    } while (0)

static const uintptr_t DEV = 0x7F0000000000, DEV_SIZE = 1 << 20, HOSTH = 0x500000000000, HOSTH_SIZE = 1 << 16,
                       DATA_BASE = 0x600000, DATA_SIZE = 4096, LOCAL = 0x10000;
static const void *P(uintptr_t v) { return (const void *)v; }

using Check = std::function<int(char *, size_t)>;

// one case, four ways; `want`: the code, `text`: what the message must contain
static void ask(const Check &check, int want, const char *text)
{
    char msg[512];
    memset(msg, 'x', sizeof msg);
    EXPECT(check(msg, sizeof msg) == want);
    EXPECT(memchr(msg, 0, sizeof msg) != nullptr);
    EXPECT(want ? strstr(msg, text) != nullptr : msg[0] == 0);
    EXPECT(check(nullptr, 0) == want);
    EXPECT(check(nullptr, 512) == want);
    char canary = 'c';
    EXPECT(check(&canary, 0) == want && canary == 'c');
    char *one = (char *)malloc(1);  // the sanitizer knows its one byte
    *one = 'x';
    EXPECT(check(one, 1) == want && *one == 0);
    free(one);
}

int main()
{
    const sos_rma_region regions[3] = {{DEV, DEV_SIZE, SOS_RMA_REGION_DEVICE_HEAP},
                                       {HOSTH, HOSTH_SIZE, SOS_RMA_REGION_HOST_HEAP},
                                       {DATA_BASE, DATA_SIZE, SOS_RMA_REGION_DATA}};
    auto layout = [&](int initialized, int my_pe, int n_pes, int mapped) {
        return sos_rma_layout{initialized, my_pe, n_pes, mapped, 3, regions};
    };
    const sos_rma_layout ok = layout(1, 1, 4, 1), down = layout(0, 1, 4, 1), unmapped = layout(1, 1, 4, 0),
                         alone = layout(1, 0, 1, 0), none = {1, 0, 4, 1, 0, nullptr};

    // ---- put / get -------------------------------------------------------------------------
    auto rma = [](const sos_rma_layout &l, sos_rma_op op) {
        return Check([=](char *m, size_t n) { return sos_rma_check(&l, &op, m, n); });
    };
    const sos_rma_op put = {P(DEV + 64), P(LOCAL), 8, 8, 8, 1, 4, 2, 1, 0};
    auto with = [](sos_rma_op op, const std::function<void(sos_rma_op &)> &f) {
        f(op);
        return op;
    };
    ask(rma(ok, put), SOS_RMA_OK, "");
    ask(rma(down, put), SOS_RMA_NOT_INITIALIZED, "not initialized");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.pe = 4; })), SOS_RMA_BAD_PE, "(4)");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.type_size = 3; })), SOS_RMA_BAD_TYPE_SIZE, "element size 3");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.strided = 1, o.local_stride = 0, o.bsize = 1; })), SOS_RMA_NOT_POSITIVE,
        "sst");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.remote = P(LOCAL); })), SOS_RMA_NOT_SYMMETRIC, "\"target\" is not");
    ask(rma(none, put), SOS_RMA_NOT_SYMMETRIC, "is not symmetric");  // a layout without regions
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.remote = P(DEV + DEV_SIZE - 4); })), SOS_RMA_NOT_SYMMETRIC, "exceeds");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.nblocks = (size_t)1 << 62; })), SOS_RMA_NOT_SYMMETRIC, "exceeds");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.put = 0, o.local = nullptr; })), SOS_RMA_NULL_LOCAL, "\"target\" is NULL");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.remote_stride = 7; })), SOS_RMA_STRIDE_LT_BSIZE, "\"tst\" (7)");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.local_stride = (ptrdiff_t)1 << 60, o.nblocks = 64; })),
        SOS_RMA_NOT_SYMMETRIC, "overflows");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.local = P(LOCAL + 2); })), SOS_RMA_BAD_TYPE_SIZE, "aligned");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.pe = 1, o.local = P(DEV + 80); })), SOS_RMA_OVERLAP, "overlaps");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.remote = P(HOSTH + 64); })), SOS_RMA_PEER_NOT_DEVICE_HEAP,
        "sym. heap region");
    ask(rma(unmapped, put), SOS_RMA_NO_PATH, "No path to peer (PE 2");
    ask(rma(ok, with(put, [](sos_rma_op &o) { o.bsize = 0, o.remote = o.local = nullptr; })), SOS_RMA_OK, "");

    // ---- atomics ---------------------------------------------------------------------------
    auto amo = [](const sos_rma_layout &l, sos_amo_op op) {
        return Check([=](char *m, size_t n) { return sos_amo_check(&l, &op, m, n); });
    };
    ask(amo(ok, {P(DEV + 64), nullptr, 8, 2, 0}), SOS_RMA_OK, "");
    ask(amo(down, {P(DEV + 64), nullptr, 8, 2, 0}), SOS_RMA_NOT_INITIALIZED, "not initialized");
    ask(amo(ok, {P(DEV + 64), nullptr, 8, -1, 0}), SOS_RMA_BAD_PE, "(-1)");
    ask(amo(ok, {nullptr, nullptr, 8, 2, 0}), SOS_RMA_NOT_SYMMETRIC, "is not symmetric");
    ask(amo(ok, {P(DEV + DEV_SIZE - 4), nullptr, 8, 2, 0}), SOS_RMA_NOT_SYMMETRIC, "exceeds device sym. heap region");
    ask(amo(ok, {P(DEV + 64), nullptr, 0, 2, 0}), SOS_RMA_BAD_TYPE_SIZE, "element size 0 is not 4 or 8");
    ask(amo(ok, {P(DEV + 68), nullptr, 8, 2, 0}), SOS_RMA_BAD_TYPE_SIZE, "\"target\"");
    ask(amo(ok, {P(DEV + 64), nullptr, 8, 2, 1}), SOS_AMO_NULL_FETCH, "\"fetch\" is NULL");
    ask(amo(ok, {P(DEV + 64), P(LOCAL + 4), 8, 2, 1}), SOS_RMA_BAD_TYPE_SIZE, "\"fetch\"");
    ask(amo(ok, {P(DATA_BASE), nullptr, 4, 0, 0}), SOS_RMA_PEER_NOT_DEVICE_HEAP, "sym. data region");
    ask(amo(unmapped, {P(DEV + 64), nullptr, 8, 2, 0}), SOS_RMA_NO_PATH, "No path");
    ask(amo(unmapped, {P(HOSTH + 8), nullptr, 8, 1, 0}), SOS_RMA_OK, "");

    // ---- put with signal -------------------------------------------------------------------
    auto psig = [](const sos_rma_layout &l, sos_put_signal_op op) {
        return Check([=](char *m, size_t n) { return sos_put_signal_check(&l, &op, m, n); });
    };
    const sos_put_signal_op ps = {P(DEV + 64), P(LOCAL), P(DEV + 4096), 8, 8, 0, 2};
    auto pwith = [](sos_put_signal_op op, const std::function<void(sos_put_signal_op &)> &f) {
        f(op);
        return op;
    };
    ask(psig(ok, ps), SOS_RMA_OK, "");
    ask(psig(down, ps), SOS_RMA_NOT_INITIALIZED, "not initialized");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.pe = 9; })), SOS_RMA_BAD_PE, "(9)");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.nelems = (size_t)1 << 62; })), SOS_RMA_NOT_SYMMETRIC, "overflows");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.target = P(LOCAL); })), SOS_RMA_NOT_SYMMETRIC, "\"target\"");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.source = nullptr; })), SOS_RMA_NULL_LOCAL, "\"source\" is NULL");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.pe = 1, o.sig_addr = P(DEV + 120); })), SOS_RMA_OVERLAP, "overlaps");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.sig_op = 2; })), SOS_SIG_BAD_OP, "(2)");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.sig_addr = P(DEV + DEV_SIZE - 4); })), SOS_RMA_NOT_SYMMETRIC,
        "\"sig_addr\"");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.sig_addr = P(DEV + 4100); })), SOS_RMA_BAD_TYPE_SIZE, "8 bytes");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.type_size = 0; })), SOS_RMA_BAD_TYPE_SIZE, "element size 0");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.target = P(DEV + 68); })), SOS_RMA_BAD_TYPE_SIZE, "Arguments");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.sig_addr = P(HOSTH + 8); })), SOS_RMA_PEER_NOT_DEVICE_HEAP,
        "\"sig_addr\"");
    ask(psig(unmapped, ps), SOS_RMA_NO_PATH, "No path");
    ask(psig(ok, pwith(ps, [](sos_put_signal_op &o) { o.nelems = 0, o.target = o.source = nullptr; })), SOS_RMA_OK, "");

    // ---- locks -----------------------------------------------------------------------------
    auto lock = [](const sos_rma_layout &l, uintptr_t p) {
        const sos_lock_op op = {P(p)};
        return Check([=](char *m, size_t n) { return sos_lock_check(&l, &op, m, n); });
    };
    ask(lock(ok, DEV + 64), SOS_RMA_OK, "");
    ask(lock(alone, DATA_BASE + 8), SOS_RMA_OK, "");
    ask(lock(down, DEV + 64), SOS_RMA_NOT_INITIALIZED, "not initialized");
    ask(lock(ok, 0), SOS_RMA_NOT_SYMMETRIC, "is not symmetric");
    ask(lock(ok, DEV + DEV_SIZE - 4), SOS_RMA_NOT_SYMMETRIC, "exceeds");
    ask(lock(alone, HOSTH + 68), SOS_RMA_BAD_TYPE_SIZE, "8 bytes");
    ask(lock(ok, HOSTH + 64), SOS_RMA_PEER_NOT_DEVICE_HEAP, "a lock shared by 4 PEs needs the device symmetric heap");
    ask(lock(unmapped, DEV + 64), SOS_RMA_NO_PATH, "the PEs' device heaps are not mapped");

    printf("onesided_checks: %d checks, %d failed%s\n", checks, failed, failed ? "" : " OK");
    return failed ? 1 : 0;
}
