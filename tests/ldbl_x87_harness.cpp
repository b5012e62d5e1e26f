// ldbl_x87_harness.cpp -- sos_amd/csrc/ldbl.h against the CPU's own x87 (tests only).
//
// Built by tests/test_ldbl_x87.py with g++ and tests/hostshim's stand-in for
// <hip/hip_runtime.h>, so the functions the kernels call (x87::min, max, add, mul) run on
// the host.  For every case `a OP b` is computed by them and by native `long double`
// (SOS's reduce_local expressions, operands through volatile so the compiler folds
// nothing); the native result's 10 value bytes are laid over a copy of `a`, which is what
// the FPU's 80-bit store leaves in a 16-byte long double.  All 16 bytes must agree.
//
//   directed  all ordered pairs of a list of encodings: exponent fields at both ends, at
//             the alignment distances of add (0..65 and past them) and around the
//             overflow/underflow edges of mul; significands with and without the integer
//             bit (denormals, pseudo-denormals, unnormals, pseudo-NaN/inf), rounding-tie
//             patterns, quiet and signalling NaN payloads; different non-zero padding in
//             `a` and `b`.
//   random    seeded; exponents near each other, near-complementary or free; random
//             integer bits; low bits masked off to force ties; b.m == a.m and
//             b.m == a.m ^ bit 62; random padding.
//
// usage: ldbl_x87_harness [--directed-only] [--random N] [--fail-fast]
// exit 0: no mismatch, 1: mismatches, 77: long double here is not the x87 80-bit type.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ldbl.h"

using sos::ld80;

#if LDBL_MANT_DIG != 64 || !(defined(__x86_64__) || defined(__i386__))
int main()
{
    printf("long double is not the x87 80-bit type here\n");
    return 77;
}
#else

static_assert(sizeof(long double) == 16 && sizeof(ld80) == 16, "16-byte long double");

enum { MIN = 0, MAX = 1, SUM = 2, PROD = 3 };
static const char *const OPNAME[4] = {"min", "max", "sum", "prod"};

static ld80 device(int op, const ld80 &a, const ld80 &b)
{
    switch (op) {
    case MIN: return sos::x87::min(a, b);
    case MAX: return sos::x87::max(a, b);
    case SUM: return sos::x87::add(a, b);
    default: return sos::x87::mul(a, b);
    }
}

static ld80 native(int op, const ld80 &a, const ld80 &b)
{
    long double xa, xb;
    memcpy(&xa, &a, 16);
    memcpy(&xb, &b, 16);
    volatile long double va = xa, vb = xb;  // 80-bit loads and stores convert nothing
    long double x = va, y = vb, r;
    switch (op) {
    case MIN: r = x < y ? x : y; break;
    case MAX: r = x > y ? x : y; break;
    case SUM: r = x + y; break;
    default: r = x * y; break;
    }
    volatile long double vr = r;
    long double out = vr;
    ld80 res = a;
    memcpy(&res, &out, 10);
    return res;
}

struct Tally {
    uint64_t cases[4] = {0, 0, 0, 0};
    uint64_t bad[4] = {0, 0, 0, 0};
    uint64_t bad_two_nans[4] = {0, 0, 0, 0};
    int shown = 0;
};

static bool fail_fast = false;

static void hex(const char *tag, const ld80 &v)
{
    printf(" %s=%04x:%016llx|%012llx", tag, (unsigned)(v.hi & 0xFFFF), (unsigned long long)v.m,
           (unsigned long long)(v.hi >> 16));
}

static void check(Tally &t, int op, const ld80 &a, const ld80 &b)
{
    const ld80 want = native(op, a, b), got = device(op, a, b);
    t.cases[op]++;
    if (memcmp(&want, &got, 16) == 0) return;
    t.bad[op]++;
    if (sos::x87::is_nan(a) && sos::x87::is_nan(b)) t.bad_two_nans[op]++;
    if (t.shown++ < 12) {
        printf("  MISMATCH %-4s", OPNAME[op]);
        hex("a", a);
        hex("b", b);
        hex("x87", want);
        hex("device", got);
        printf("\n");
    }
    if (fail_fast) {
        printf("FAIL: stopped at the first mismatch\n");
        exit(1);
    }
}

static uint64_t report(const char *set, const Tally &t)
{
    uint64_t bad = 0;
    for (int op = 0; op < 4; op++) {
        printf("%s %-4s: %llu cases, %llu mismatches (%llu with two NaN operands)\n", set, OPNAME[op],
               (unsigned long long)t.cases[op], (unsigned long long)t.bad[op],
               (unsigned long long)t.bad_two_nans[op]);
        bad += t.bad[op];
    }
    return bad;
}

// ------------------------------------------------------------------------------------
static const int BIAS = 16383;

static std::vector<uint32_t> directed_exponents()
{
    // both ends first: with --fail-fast a broken NaN, overflow or denormal rule shows at once
    std::vector<uint32_t> e = {0x7FFF, 0x7FFE, 0x7FFD, 0, 1, 2, 63, 64, 65, 127, 128, 129};
    for (int k = BIAS - 65; k <= BIAS + 1; k++) e.push_back((uint32_t)k);
    for (uint32_t k : {0x403Eu, 0x403Fu, 0x4040u, 0x1FFFu, 0x2000u, 0x5FFFu, 0x6000u}) e.push_back(k);
    return e;
}

static const uint64_t DIRECTED_SIGNIFICANDS[] = {
    // integer bit clear: zero, the smallest denormals; with a non-zero exponent unnormals,
    // with 0x7FFF pseudo-infinity and pseudo-NaNs
    0x0000000000000000ull, 0x0000000000000001ull, 0x0000000000000002ull, 0x0000000000000003ull,
    0x4000000000000000ull, 0x7FFFFFFFFFFFFFFFull, 0x4000000000000001ull, 0x0000000080000000ull,
    // integer bit set: 1.0, one ulp above, all ones, with and without the low bit; with
    // exponent 0 pseudo-denormals, with 0x7FFF infinity and signalling NaNs
    0x8000000000000000ull, 0x8000000000000001ull, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFEull,
    0x8000000000000002ull, 0x8000000000000003ull,
    // products and sums that end exactly on a tie, above an even and above an odd result
    0x8000000080000000ull, 0xC000000080000000ull, 0xFFFFFFFF80000000ull, 0x8000000100000000ull,
    0xAAAAAAAAAAAAAAAAull, 0xD555555555555555ull,
    // NaN payloads: quiet and signalling, pairs that differ in bit 62 only
    0xC000000000000000ull, 0xC000000000000001ull, 0xC000000000000123ull, 0x8000000000000123ull,
    0xBFFFFFFFFFFFFFFFull, 0xA000000000000000ull, 0xE000000000000000ull,
};

static const uint64_t PAD_A = 0xA1B2C3D4E5F6ull, PAD_B = 0x0718293A4B5Cull;

static uint64_t run_directed()
{
    const std::vector<uint32_t> exps = directed_exponents();
    std::vector<ld80> v;
    for (uint32_t e : exps)
        for (uint64_t m : DIRECTED_SIGNIFICANDS)
            for (uint32_t sign = 0; sign < 2; sign++) v.push_back(ld80{m, (uint64_t)((sign << 15) | e)});
    printf("directed: %zu encodings (2 signs x %zu exponent fields x %zu significands), all ordered pairs\n",
           v.size(), exps.size(), sizeof(DIRECTED_SIGNIFICANDS) / sizeof(uint64_t));
    Tally t;
    for (const ld80 &x : v) {
        const ld80 a{x.m, x.hi | (PAD_A << 16)};
        for (const ld80 &y : v) {
            const ld80 b{y.m, y.hi | (PAD_B << 16)};
            for (int op = 0; op < 4; op++) check(t, op, a, b);
        }
    }
    return report("directed", t);
}

// ------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()  // splitmix64
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint32_t clamp_exp(int e) { return (uint32_t)(e < 0 ? 0 : e > 0x7FFF ? 0x7FFF : e); }

static uint32_t random_exp()
{
    const uint64_t r = rnd();
    switch (r & 15) {
    case 0: return 0;
    case 1: return 0x7FFF;
    case 2: return 1 + (uint32_t)((r >> 8) % 70);
    case 3: return 0x7FFE - (uint32_t)((r >> 8) % 3);
    default: return 1 + (uint32_t)((r >> 8) % 0x7FFE);
    }
}

static uint64_t random_significand()
{
    uint64_t r = rnd(), m = rnd();
    if (r & 1) m |= 1ull << 63;                                  // else: a random integer bit
    if (r & 2) m &= ~0ull << ((r >> 8) % 64);                    // trailing zeros: ties
    if ((r & 12) == 12) m = (m & (1ull << 63)) | ((r >> 16) & 3);  // next to a power of two
    return m;
}

static uint64_t run_random(uint64_t n)
{
    printf("random: %llu cases, seed %016llx\n", (unsigned long long)n, (unsigned long long)rng_state);
    Tally t;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t r = rnd();
        const uint32_t ea = random_exp();
        uint32_t eb;
        const int jitter = (int)((r >> 8) % 141) - 70;
        switch ((r >> 4) % 3) {
        case 0: eb = clamp_exp((int)ea + jitter); break;                          // add: aligned
        case 1: {                                                                   // mul: the edges
            static const int sums[3] = {BIAS, 2 * BIAS, 3 * BIAS};                  // of its range
            eb = clamp_exp(sums[(r >> 16) % 3] - (int)ea + jitter);
            break;
        }
        default: eb = random_exp(); break;
        }
        const uint64_t ma = random_significand();
        uint64_t mb = random_significand();
        if (((r >> 20) & 15) == 0) mb = ma;
        if (((r >> 20) & 15) == 1) mb = ma ^ (1ull << 62);
        const ld80 a{ma, (rnd() << 16) | (uint32_t)(((r >> 24) & 1) << 15) | ea};
        const ld80 b{mb, (rnd() << 16) | (uint32_t)(((r >> 25) & 1) << 15) | eb};
        check(t, (int)(k & 3), a, b);
    }
    return report("random", t);
}

int main(int argc, char **argv)
{
    uint64_t nrandom = 24000000;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--directed-only")) nrandom = 0;
        else if (!strcmp(argv[i], "--fail-fast")) fail_fast = true;
        else if (!strcmp(argv[i], "--random") && i + 1 < argc) nrandom = strtoull(argv[++i], nullptr, 10);
        else {
            fprintf(stderr, "usage: %s [--directed-only] [--random N] [--fail-fast]\n", argv[0]);
            return 2;
        }
    }
    uint64_t bad = run_directed();
    if (nrandom) bad += run_random(nrandom);
    printf("%s: %llu mismatches\n", bad ? "FAIL" : "OK", (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
