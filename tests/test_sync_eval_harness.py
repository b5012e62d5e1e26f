"""CPU: the host-only part of put-with-signal and the point-to-point waits as a program of
its own.  tests/sync_eval_harness.cpp (its own main; compiled together with
sos_amd/csrc/onesided_checks.cpp, no HIP, no Python process, nothing preloaded) sweeps
sos_sync_eval against a model of SOS's loops, both check functions over hand-built layouts and
the copy split of sosx_put_signal; it runs plain and under AddressSanitizer + UBSan, with
buffers of the exact extents."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "sync_eval_harness.cpp"), os.path.join(ROOT, "sos_amd", "csrc", "onesided_checks.cpp")]
INCLUDES = [f"-I{ROOT}/include", f"-I{ROOT}/sos_amd/csrc"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build_and_run(tmp_path, name, flags, env=None):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", *flags, *INCLUDES, *SRCS, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "sync eval, checks and put_signal plans OK" in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_sync_eval_harness(tmp_path):
    build_and_run(tmp_path, "sync_eval_harness", ["-O2"])


def test_sync_eval_harness_under_asan(tmp_path):
    build_and_run(tmp_path, "sync_eval_harness_asan", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  env={"ASAN_OPTIONS": "detect_leaks=1"})
