"""CPU: every refusal of the one-sided layer's argument checks, frozen.

(a) tests/golden/onesided_refusals.json records what sos_rma_check, sos_amo_check,
    sos_put_signal_check, sos_sync_check and sos_lock_check answered -- the code and the message
    bytes -- for a fixed grid of cases at the commit the file names (tests/golden/make_refusals.py).
    The built library must answer every case the same.  A case that differs is a change of
    behaviour in sos_amd/csrc/onesided_checks.cpp, not a fixture to regenerate.
(b) tests/onesided_checks_harness.cpp, a program of its own compiled with onesided_checks.cpp --
    no HIP, no library, nothing preloaded -- plain and with -fsanitize=address,undefined: the four
    layout-based checks with msg == NULL, n == 0 and a one-byte buffer, the paths REFUSE guards.
Nothing is started that could abort."""
import collections
import json
import os
import subprocess
import sys

import pytest

from sos_amd import shmem as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(ROOT, "tests", "build")
CSRC = os.path.join(ROOT, "sos_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_refusals as M  # noqa: E402

FLAVOURS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "onesided_refusals.json")) as f:
        return json.load(f)


def test_record_is_the_grid_of_a_commit(record):
    assert len(record["commit"]) == 40 and record["msg_len"] == M.MSG_LEN
    assert [tuple(r) for r in record["regions"]] == M.REGIONS
    grid = []
    for fn, cases in M.GRID:
        for lay, op in cases():
            if [fn, lay, op] not in grid:
                grid.append([fn, lay, op])
    assert [c[:3] for c in record["cases"]] == grid           # the script's grid, all of it, in its order
    per_fn = collections.Counter(c[0] for c in record["cases"])
    assert set(per_fn) == set(M.OPS) and min(per_fn.values()) >= 80
    # every refusal code of the five checks is in the record, and so is acceptance
    codes = {(c[0], c[3]) for c in record["cases"]}
    want = {"sos_rma_check": range(11), "sos_amo_check": (0, 1, 2, 4, 8, 9, 10, 11),
            "sos_put_signal_check": (0, 1, 2, 4, 5, 7, 8, 9, 10, 12), "sos_sync_check": (0, 1, 4, 5, 7, 10, 13),
            "sos_lock_check": (0, 1, 4, 8, 9, 10)}
    for fn, cs in want.items():
        assert {c for f, c in codes if f == fn} == set(cs), fn


@pytest.mark.parametrize("fn", list(M.OPS))
def test_library_answers_as_recorded(record, fn):
    lib = S.lib()
    differ = []
    for f, lay, op, code, msg in record["cases"]:
        if f == fn and M.call(lib, f, lay, op) != (code, msg):
            differ.append((lay, op, (code, msg), M.call(lib, f, lay, op)))
    assert not differ, f"{len(differ)} cases differ from commit {record['commit'][:7]}; the first: {differ[0]}"


@pytest.fixture(scope="module", params=list(FLAVOURS))
def harness(request):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, f"onesided_checks_harness_{request.param}")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *FLAVOURS[request.param], "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "onesided_checks_harness.cpp"),
           os.path.join(CSRC, "onesided_checks.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_harness_passes(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=120, env=dict(os.environ, **ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-4000:]
    assert " 0 failed OK" in r.stdout, r.stdout
    assert int(r.stdout.split(":")[1].split()[0]) == 7 * 52, r.stdout  # 7 EXPECTs for each of the 52 cases
