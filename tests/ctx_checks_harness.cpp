// ctx_checks_harness.cpp -- a program of its own over the plain check functions of the
// communication contexts (sos_amd/csrc/onesided_checks.cpp, compiled next to it; no HIP, no
// library): the option mask, invalid / default / destroyed / unknown handles, the team-index
// translation for a strided team, the SHMEMX_CTX_STREAMS values and the stream-pool
// assignment.  Built plain and with the address and undefined-behaviour sanitizers
// (tests/test_ctx_checks.py).  Handles are made-up numbers: a check that dereferenced one
// would fault, and the sanitizer would say where.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "api_internal.h"

static int checks = 0, failed = 0;

#define EXPECT(cond)                                                       \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            ++failed;                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
        }                                                                  \
    } while (0)

static const void *H(uintptr_t v) { return (const void *)v; }

int main()
{
    char msg[256];
    // ---- options ---------------------------------------------------------------------
    for (long o = 0; o < 8; ++o) EXPECT(sos_ctx_options_check(o, msg, sizeof msg) == SOS_CTX_OK && !msg[0]);
    EXPECT(SHMEM_CTX_PRIVATE == 1 && SHMEM_CTX_SERIALIZED == 2 && SHMEM_CTX_NOSTORE == 4);
    for (long o : {8L, 9L, 1L << 20, -1L, (long)(1ul << 63)}) {
        EXPECT(sos_ctx_options_check(o, msg, sizeof msg) == SOS_CTX_BAD_OPTIONS);
        EXPECT(strstr(msg, "\"options\"") && strstr(msg, "SHMEM_CTX_NOSTORE"));
    }
    EXPECT(sos_ctx_options_check(8, nullptr, 0) == SOS_CTX_BAD_OPTIONS);  // no message buffer

    // ---- handles: 8 PEs; the default context, a world context, one on the strided team
    // (start 1, stride 2, size 3), two destroyed ----------------------------------------
    const std::vector<sos_ctx_entry> live = {{H(0x1000), 0, 1, 8}, {H(0x2000), 0, 1, 8}, {H(0x3000), 1, 2, 3}};
    const std::vector<const void *> dead = {H(0x4000), H(0x5000)};
    const sos_ctx_table t = {(int)live.size(), live.data(), (int)dead.size(), dead.data()};
    int index = 7, pe = 0;
    EXPECT(sos_ctx_check(&t, nullptr, &pe, &index, msg, sizeof msg) == SOS_CTX_INVALID && index == -1);
    EXPECT(strstr(msg, "SHMEM_CTX_INVALID"));
    EXPECT(sos_ctx_check(&t, H(0x4000), &pe, &index, msg, sizeof msg) == SOS_CTX_DESTROYED && index == -1);
    EXPECT(strstr(msg, "destroyed") && strstr(msg, "0x4000"));
    EXPECT(sos_ctx_check(&t, H(0x5000), nullptr, nullptr, msg, sizeof msg) == SOS_CTX_DESTROYED);
    EXPECT(sos_ctx_check(&t, H(0x6000), &pe, &index, msg, sizeof msg) == SOS_CTX_UNKNOWN && index == -1);
    EXPECT(strstr(msg, "not a context"));
    EXPECT(sos_ctx_check(&t, H(0x1008), &pe, &index, msg, sizeof msg) == SOS_CTX_UNKNOWN);  // inside an object
    EXPECT(pe == 0);  // a refusal leaves the PE alone
    // the default context: accepted, world PEs unchanged
    for (int p = 0; p < 8; ++p) {
        pe = p;
        EXPECT(sos_ctx_check(&t, H(0x1000), &pe, &index, msg, sizeof msg) == SOS_CTX_OK && index == 0 && pe == p && !msg[0]);
    }
    EXPECT(sos_ctx_check(&t, H(0x1000), nullptr, &index, msg, sizeof msg) == SOS_CTX_OK && index == 0);  // quiet / fence
    EXPECT(sos_ctx_check(&t, H(0x2000), nullptr, nullptr, nullptr, 0) == SOS_CTX_OK);
    for (int bad : {-1, 8, 1 << 30}) {
        pe = bad;
        EXPECT(sos_ctx_check(&t, H(0x2000), &pe, &index, msg, sizeof msg) == SOS_CTX_BAD_PE && pe == bad);
        char want[64];
        snprintf(want, sizeof want, "PE argument (%d) is invalid", bad);
        EXPECT(!strcmp(msg, want));  // put / get's own message
    }
    // the strided team: indices 0, 1, 2 are PEs 1, 3, 5; index 3 is refused
    const int want_pe[3] = {1, 3, 5};
    for (int i = 0; i < 3; ++i) {
        pe = i;
        EXPECT(sos_ctx_check(&t, H(0x3000), &pe, &index, msg, sizeof msg) == SOS_CTX_OK && index == 2 && pe == want_pe[i]);
    }
    for (int bad : {3, 5, -1}) {  // 5 is a member's world PE, not an index
        pe = bad;
        EXPECT(sos_ctx_check(&t, H(0x3000), &pe, &index, msg, sizeof msg) == SOS_CTX_BAD_PE && pe == bad);
    }
    EXPECT((int)SOS_CTX_BAD_PE == (int)SOS_RMA_BAD_PE);
    // an empty table refuses everything but faults on nothing
    const sos_ctx_table none = {0, nullptr, 0, nullptr};
    EXPECT(sos_ctx_check(&none, H(0x1000), &pe, &index, msg, sizeof msg) == SOS_CTX_UNKNOWN);
    // a reused address is live again: the live list is looked at first
    const std::vector<const void *> dead2 = {H(0x2000)};
    const sos_ctx_table reused = {(int)live.size(), live.data(), 1, dead2.data()};
    pe = 2;
    EXPECT(sos_ctx_check(&reused, H(0x2000), &pe, &index, msg, sizeof msg) == SOS_CTX_OK && index == 1 && pe == 2);

    // ---- SHMEMX_CTX_STREAMS ------------------------------------------------------------
    EXPECT(sos_ctx_pool_size(nullptr, msg, sizeof msg) == 3 && sos_ctx_pool_size("", msg, sizeof msg) == 3);
    EXPECT(sos_ctx_pool_size("1", msg, sizeof msg) == 1 && sos_ctx_pool_size("3", msg, sizeof msg) == 3);
    EXPECT(sos_ctx_pool_size("31", msg, sizeof msg) == 31 && !msg[0]);
    for (const char *bad : {"0", "32", "-1", "x", "3x", "99999999999999999999"}) {
        EXPECT(sos_ctx_pool_size(bad, msg, sizeof msg) == -1);
        EXPECT(strstr(msg, "SHMEMX_CTX_STREAMS") && strstr(msg, "1..31"));
    }
    // ---- pool assignment: round-robin, so more contexts than streams share -------------
    for (unsigned long n = 0; n < 10; ++n) EXPECT(sos_ctx_stream_slot(n, 1) == 0);
    const int want3[7] = {0, 1, 2, 0, 1, 2, 0};
    for (unsigned long n = 0; n < 7; ++n) EXPECT(sos_ctx_stream_slot(n, 3) == want3[n]);
    EXPECT(sos_ctx_stream_slot(0, 3) != sos_ctx_stream_slot(1, 3));  // the first two contexts: two streams
    EXPECT(sos_ctx_stream_slot(3, 3) == sos_ctx_stream_slot(0, 3));  // the fourth shares the first's
    for (unsigned long n : {0ul, 30ul, 31ul, 62ul, ~0ul}) {
        const int s = sos_ctx_stream_slot(n, 31);
        EXPECT(s >= 0 && s < 31 && s == (int)(n % 31));
    }
    EXPECT(sos_ctx_stream_slot(5, 0) == 0);  // never an index outside a pool
    printf("ctx_checks: %d checks, %d failed%s\n", checks, failed, failed ? "" : " OK");
    return failed ? 1 : 0;
}
