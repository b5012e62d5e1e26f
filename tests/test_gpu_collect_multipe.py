"""GPU, several PE processes on one MI355X: fcollect, alltoall and alltoalls through the
public API (tests/collect_check_pe.py) over the p2p transport (stream and host
signalling), a single PE, and the RCCL executor through the file-based stand-in
(tests/fakerccl), plus the C example examples/alltoall_types.c."""
import glob
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSHRUN = os.path.join(ROOT, "tools", "oshrun")
FAKE = os.path.join(ROOT, "tests", "fakerccl", "libsos_amd_fakerccl.so")
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "collect_check_pe.py")]


def _base_env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def oshrun(np_, cmd, timeout=300, extra_env=None):
    """The p2p runs of tests/test_gpu_multipe.py: same environment, same queue rule at 8."""
    env = _base_env()
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M",
                "SHMEMX_STAGE_BYTES": "64M", "SHMEMX_DEVICE": "0", "PYTHONPATH": ROOT})
    if np_ >= 8:
        env["GPU_MAX_HW_QUEUES"] = "1"  # eight PE processes on one GPU: one hardware queue each
    env.update(extra_env or {})
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30),
                           *cmd], capture_output=True, text=True, timeout=timeout, env=env)


def oshrun_fake(np_, cmd, timeout=300, **extra):
    """The RCCL-executor runs of tests/test_gpu_fakerccl.py: same environment."""
    env = _base_env()
    env.update({"SOSX_LIBRARY": FAKE, "SHMEMX_TRANSPORT": "rccl", "SHMEMX_DEVICE": "0",
                "SHMEMX_DEVICE_HEAP_SIZE": "256M", "FAKERCCL_TIMEOUT": "60", "FAKERCCL_STATS": "1",
                "PYTHONPATH": ROOT})
    env.update(extra)
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30),
                           *cmd], capture_output=True, text=True, timeout=timeout, env=env)


def _all_ok(r, np_):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(r"PE (\d+)/\d+: (\d+) checks OK \(p2p signal (\w+)\)", r.stdout)
    assert sorted(int(p) for p, _, _ in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    assert all(int(c) > 100 for _, c, _ in ok), ok
    return ok


@pytest.mark.parametrize("np_,signal", [(2, "stream"), (3, "stream"), (4, "stream"), (8, "stream"),
                                        (3, "host"), (1, "host")])
def test_collect_check_p2p(np_, signal):
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal})
    ok = _all_ok(r, np_)
    if np_ > 1:
        assert {m for _, _, m in ok} == {signal}, ok


@pytest.fixture
def no_leftover_messages():
    assert os.path.exists(FAKE), "tests/fakerccl/libsos_amd_fakerccl.so is not built"
    yield
    left = glob.glob("/dev/shm/fakerccl_*")
    for f in left:
        os.unlink(f)
    assert not left, f"unreceived messages: {left[:4]}"


def _used_fake(r, np_):
    assert "fakerccl error" not in r.stderr, r.stderr[-2000:]
    sent = {int(rk): int(m) for rk, m in
            re.findall(r"fakerccl stats: rank (\d+) sent (\d+) messages", r.stderr)}
    assert sorted(sent) == list(range(np_)) and min(sent.values()) > 0, r.stderr[-2000:]


@pytest.mark.parametrize("np_", [2, 3])
def test_collect_check_rccl_executor(no_leftover_messages, np_):
    r = oshrun_fake(np_, PE_SCRIPT)
    _all_ok(r, np_)
    _used_fake(r, np_)


def test_collect_check_rccl_native_allgather(no_leftover_messages, np_=2):
    """SHMEMX_RCCL_ALLGATHER=1: fcollect's second round is the equal-chunk allgather the
    RCCL executor hands to ncclAllGather (counted by the stand-in)."""
    r = oshrun_fake(np_, PE_SCRIPT, SHMEMX_RCCL_ALLGATHER="1")
    _all_ok(r, np_)
    _used_fake(r, np_)
    ag = {int(rk): int(a) for rk, a in
          re.findall(r"fakerccl stats: rank (\d+) sent \d+ messages, \d+ bytes, (\d+) allgathers",
                     r.stderr)}
    assert sorted(ag) == list(range(np_)) and min(ag.values()) > 0, r.stderr[-2000:]


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.mark.parametrize("np_", [2, 4])
def test_alltoall_types_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "alltoall_types")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"alltoall_types: OK ({np_} PEs)" in r.stdout
