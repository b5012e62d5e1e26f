"""CPU: the host split of the block-strided copy (sos_amd/csrc/blockcopy_plan.h).

tests/blockcopy_plan.cpp sweeps every element size, block sizes around one and 64 16-B
vectors, 1 / 2 / 3 / 257 blocks, strides equal to the block, one more, a multiple of 16 B
and 4099, and every pair of base misalignments; a CPU interpreter walks each plan as the
kernel's workgroups do and must move exactly the bytes of the definition, each once, with
every access inside a block and aligned.  The program (host code with its own main, no
HIP) runs plain and under AddressSanitizer + UBSan; the buffers have the exact extents.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "blockcopy_plan.cpp")
INCLUDES = [f"-I{ROOT}/tests/hostshim", f"-I{ROOT}/include", f"-I{ROOT}/sos_amd/csrc"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build_and_run(tmp_path, name, flags, env=None):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-g", "-pthread", *flags, *INCLUDES, SRC, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "block copy plans OK" in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_blockcopy_plan_sweep(tmp_path):
    out = build_and_run(tmp_path, "blockcopy_plan", ["-O2"])
    assert "194432 cases" in out, out  # the whole cross product ran


def test_blockcopy_plan_sweep_under_asan(tmp_path):
    build_and_run(tmp_path, "blockcopy_plan_asan",
                  ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  env={"ASAN_OPTIONS": "detect_leaks=1"})


def test_library_plan_matches_header():
    """sosx_block_copy_plan (the library's own view) names the three regimes and the
    delegated forms for one shape each, without touching a device."""
    import ctypes

    from sos_amd import shmem as S
    f = S.lib().sosx_block_copy_plan
    out = (ctypes.c_longlong * 8)()

    def plan(dst, dstr, src, sstr, bsize, nblocks, es):
        assert f(dst, dstr, src, sstr, bsize, nblocks, es, out) == 0
        return list(out)

    base = 1 << 20
    # congruent: 100 floats at +8, strides 128 floats: head 8 B, 24 vectors, tail 8 B
    assert plan(base + 8, 128, 2 * base + 8, 256, 100, 300, 4)[:6] == [4, 16, 0, 8, 24, 8]
    # incongruent, target stride on the 16-B grid, source 4 B off: unaligned 16-B loads
    assert plan(base, 128, 2 * base + 4, 101, 100, 300, 4)[:6] == [5, 16, 1, 0, 25, 0]
    # incongruent, target stride off the grid: the common width (4 B)
    assert plan(base, 101, 2 * base, 128, 100, 300, 4)[:6] == [5, 4, 0, 0, 100, 0]
    # 2-byte elements at an odd element offset: 2-B accesses, no unaligned loads
    assert plan(base + 2, 64, 2 * base, 64, 40, 9, 2)[:3] == [5, 2, 0]
    # small blocks (iput with both sides strided): one lane per element
    assert plan(base, 3, 2 * base, 5, 1, 1000, 4)[:3] == [3, 4, 0]
    # single elements, one side contiguous: sosx_strided_copy's pack / unpack
    assert plan(base, 1, 2 * base, 5, 1, 1000, 4)[0] == 2
    # blocks that abut on both sides: one contiguous run
    assert plan(base, 7, 2 * base, 7, 7, 1000, 4)[0] == 1
    # more than one workgroup for 300 blocks of 24 / 25 vectors
    assert plan(base + 8, 128, 2 * base + 8, 256, 100, 300, 4)[6:] == [8, 2]
    assert f(base, 3, 2 * base, 5, 4, 10, 4, out) == -3  # stride < bsize
