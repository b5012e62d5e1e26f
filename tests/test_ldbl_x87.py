"""CPU: sos_amd/csrc/ldbl.h (x87 80-bit arithmetic in integer code) against the CPU's FPU.

tests/ldbl_x87_harness.cpp includes the header the kernels include (tests/hostshim stands
in for <hip/hip_runtime.h>) and compares x87::min / max / add / mul with native
`long double` over a directed all-pairs set and a seeded random set, all 16 bytes of
every result, under UBSan (the shift counts of round_pack and add).

The mutants check the checker: each is the header with one rule of the arithmetic broken
(a rounding tie, the carry out of 64 bits, the step into the smallest normal, overflow by
rounding, the sticky borrow, the NaN choice, ...), and the directed set alone must
report it.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sos_amd", "csrc", "ldbl.h")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build(exe, header_dir):
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                        f"-I{ROOT}/tests/hostshim", f"-I{header_dir}", f"{ROOT}/tests/ldbl_x87_harness.cpp",
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def run(exe, *args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    if r.returncode == 77:
        pytest.skip("long double is not the x87 80-bit type on this machine")
    return r


def test_ldbl_matches_x87(tmp_path):
    exe = tmp_path / "ldbl_x87"
    build(exe, os.path.dirname(HEADER))
    r = run(exe)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    for s in ("directed", "random"):
        for op in ("min ", "max ", "sum ", "prod"):
            assert any(l.startswith(f"{s} {op}:") and ", 0 mismatches" in l for l in r.stdout.splitlines()), (s, op)
    assert "OK: 0 mismatches" in r.stdout


# (name, text in ldbl.h, its replacement): one broken rule each
MUTANTS = [
    ("tie_to_even", "if (round && (sticky || (m & 1))) {", "if (round && sticky) {"),
    ("tie_always_up", "if (round && (sticky || (m & 1))) {", "if (round) {"),
    ("carry_out_of_64", "            biased += 1;\n", ""),
    ("into_smallest_normal", "biased = 1;  // rounded up into the smallest normal", "biased = 0;"),
    ("overflow_by_rounding", "if (biased >= 0x7FFF) return", "if (biased > 0x7FFF) return"),
    ("sticky_borrow", "if (sticky) S -= 1;", ""),
    ("shifted_operand_sticky", "sticky = (B & ((((u128)1) << d) - 1)) != 0;", "sticky = false;"),
    ("denormal_sticky", "sticky |= (S & ((((u128)1) << sh) - 1)) != 0;", ""),
    ("denormal_scale", "if (e == 0) e = 1;\n    return e - 16383 - 63;", "return e - 16383 - 63;"),
    ("cancellation_sign", "return make(a, 0, 0);  // exact cancellation", "return make(a, s1 << 15, 0);  //"),
    ("zero_sum_sign", "return make(a, (sa & sb) << 15, 0);", "return make(a, sa << 15, 0);"),
    ("nan_raw_compare", "b.m > a.m || (b.m == a.m", "(b.m | (1ull << 62)) > (a.m | (1ull << 62)) || (b.m == a.m"),
    ("nan_equal_sign", "(b.m == a.m && (se(a) >> 15))", "false"),
    ("nan_quieting", "return make(a, se(w), w.m | (1ull << 62));", "return make(a, se(w), w.m);"),
    ("pseudo_denormal_unsupported", "return e != 0 && !(a.m >> 63);", "return (e != 0) != (bool)(a.m >> 63);"),
    ("signed_zero_compare", "    if (is_zero(a) && is_zero(b)) return false;\n", ""),
    ("minmax_padding", "const ld80 &c = gt(b, a) ? a : b;\n    return make(a, se(c), c.m);",
     "const ld80 &c = gt(b, a) ? a : b;\n    return c;"),
    ("inf_times_zero", "if (is_zero(a) || is_zero(b)) return default_nan(a);", ""),
]


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_directed_set_catches_mutant(tmp_path, name, old, new):
    text = open(HEADER).read()
    assert text.count(old) == 1, f"mutant {name}: its text is no longer in ldbl.h exactly once"
    (tmp_path / "ldbl.h").write_text(text.replace(old, new))
    exe = tmp_path / "ldbl_x87_mutant"
    build(exe, tmp_path)
    r = run(exe, "--directed-only", "--fail-fast")
    assert r.returncode == 1, f"mutant {name} passed the directed set:\n" + r.stdout[-2000:] + r.stderr[-2000:]
    assert "MISMATCH" in r.stdout
