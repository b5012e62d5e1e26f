"""CPU: the host split of the p2p transport's gather (sos_amd/csrc/gather_plan.h).

tests/gather_plan.cpp sweeps single segments (every source / destination offset pair mod
16, both settings of the unaligned-load switch, sizes around one 16-B vector and around one
tile) and segment lists (0 to 40 segments with five patterns of empty ones, with and
without a gate); a CPU interpreter walks every launch as k_gather's workgroups do, in the
three load forms, and must write every destination byte exactly once with its source byte,
keep every access inside its segment (aligned loads: at least one byte of it), find each
live segment in exactly one launch and the gate where the rule puts it.  The program (host
code with its own main, no HIP) runs plain and under AddressSanitizer + UBSan; the buffers
have the exact extents.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gather_plan.cpp")
INCLUDES = [f"-I{ROOT}/tests/hostshim", f"-I{ROOT}/include", f"-I{ROOT}/sos_amd/csrc"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build_and_run(tmp_path, name, flags, env=None):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-g", *flags, *INCLUDES, SRC, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "gather plans OK" in r.stdout, r.stdout[-2000:]
    return r.stdout


@needs_gxx
def test_gather_plan_sweep(tmp_path):
    out = build_and_run(tmp_path, "gather_plan", ["-O2"])
    # 16 x 16 offset pairs x 2 x 13 sizes + 8 lists x 5 patterns x 2 x 2: the whole sweep ran
    assert "6816 cases" in out, out


@needs_gxx
def test_gather_plan_sweep_under_asan(tmp_path):
    build_and_run(tmp_path, "gather_plan_asan",
                  ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  env={"ASAN_OPTIONS": "detect_leaks=1"})


def test_library_plan_matches_header():
    """sosx_gather_plan (the library's own view, no device touched): one shape per gate
    placement, and the 20-segment list whose first 4 segments are empty -- 16 live segments
    that fit ONE launch, each packed once."""
    from sos_amd import _lib
    tile = 256 * 4 * 16  # kTileVec vectors of 16 B
    base = 1 << 30

    def plan(segs, gated):
        srcs = [base + (i << 24) + so for i, (so, _, _) in enumerate(segs)]
        dsts = [2 * base + (i << 24) + do for i, (_, do, _) in enumerate(segs)]
        return _lib.gather_plan(srcs, dsts, [n for _, _, n in segs], gated)

    NONE, FUSED, BEFORE, ALONE = 0, 1, 2, 3
    # fused: three small segments, one launch of 0 + 3 + 1 tiles
    p = plan([(1, 2, 1), (5, 0, 40000), (0, 7, 100)], True)
    assert p == dict(launches=1, tiles=4, live=3, slots=3, gate=FUSED, first_blocks=4, last_blocks=4)
    assert plan([(1, 2, 1), (5, 0, 40000), (0, 7, 100)], False)["gate"] == NONE
    # exactly kGateMaxBlocks tiles still fuse; one more does not
    assert plan([(0, 0, 16 * tile)], True)["gate"] == FUSED
    p = plan([(0, 0, 16 * tile + 16)], True)
    assert (p["launches"], p["tiles"], p["gate"]) == (1, 17, BEFORE)
    p = plan([(3, 3, 17 * tile + 5)], True)  # head 13 B: 17 tiles less one vector
    assert (p["launches"], p["tiles"], p["gate"]) == (1, 17, BEFORE)
    # own step because of the count: 17 small segments are two launches
    p = plan([(i % 16, (3 * i) % 16, 100 + i) for i in range(17)], True)
    assert p == dict(launches=2, tiles=17, live=17, slots=17, gate=BEFORE, first_blocks=16, last_blocks=1)
    # nothing copied: the step alone (and no launch at all without a gate)
    assert plan([(0, 0, 0)] * 5, True) == dict(launches=0, tiles=0, live=0, slots=0, gate=ALONE,
                                               first_blocks=0, last_blocks=0)
    assert plan([], True)["gate"] == ALONE and plan([], False)["gate"] == NONE
    # a segment shorter than its head has no tile: the grid is still one workgroup
    p = plan([(0, 9, 5)], True)
    assert (p["tiles"], p["first_blocks"], p["gate"]) == (0, 1, FUSED)
    # 20 segments, the first 4 empty: 16 live ones in ONE launch, none packed twice
    segs = [(i % 16, (5 * i) % 16, 0 if i < 4 else 1000 + i) for i in range(20)]
    for gated in (False, True):
        p = plan(segs, gated)
        assert (p["launches"], p["live"], p["slots"]) == (1, 16, 16), p
        assert p["gate"] == (FUSED if gated else NONE)
    # empties anywhere: slots == live, launches == ceil(live / 16)
    segs = [(i % 16, (7 * i) % 16, 0 if i % 2 == 0 else 50 + i) for i in range(40)]
    p = plan(segs, True)
    assert (p["launches"], p["live"], p["slots"], p["gate"]) == (2, 20, 20, BEFORE)
    assert _lib.lib().sosx_gather_plan(-1, None, None, None, 0, (ctypes.c_longlong * 8)()) == -3
    assert _lib.lib().sosx_gather_plan(0, None, None, None, 0, None) == -3
