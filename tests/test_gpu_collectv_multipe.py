"""GPU, several PE processes on one MI355X: shmem_collect through the public API
(tests/collectv_check_pe.py) over the p2p transport (stream and host signalling), a
single PE, and the RCCL executor through the file-based stand-in (tests/fakerccl), plus
the C example examples/collect_ragged.c.  Helpers follow tests/test_gpu_collect_multipe.py."""
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
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "collectv_check_pe.py")]


def _base_env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def oshrun(np_, cmd, timeout=300, extra_env=None):
    env = _base_env()
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M",
                "SHMEMX_STAGE_BYTES": "64M", "SHMEMX_DEVICE": "0", "PYTHONPATH": ROOT})
    if np_ >= 8:
        env["GPU_MAX_HW_QUEUES"] = "1"  # eight PE processes on one GPU: one hardware queue each
    env.update(extra_env or {})
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30),
                           *cmd], capture_output=True, text=True, timeout=timeout, env=env)


def oshrun_fake(np_, cmd, timeout=300, **extra):
    env = _base_env()
    env.update({"SOSX_LIBRARY": FAKE, "SHMEMX_TRANSPORT": "rccl", "SHMEMX_DEVICE": "0",
                "SHMEMX_DEVICE_HEAP_SIZE": "256M", "FAKERCCL_TIMEOUT": "60", "FAKERCCL_STATS": "1",
                "PYTHONPATH": ROOT})
    env.update(extra)
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30),
                           *cmd], capture_output=True, text=True, timeout=timeout, env=env)


def _all_ok(r, np_, small_off=False):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(r"PE (\d+)/\d+: (\d+) checks OK \(p2p signal (\w+), (\d+) peer reads, 0 unacquired, "
                    r"(\d+) small, (\d+) executor\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    assert all(int(m[1]) > 100 for m in ok), ok
    # each call's path was checked against the caps inside the run (sosx_small_collect_calls);
    # here: both paths were really exercised
    for m in ok:
        small, executor = int(m[4]), int(m[5])
        if np_ == 1 or small_off:
            assert small == 0 and executor > 0, ok
        else:
            assert small > 0 and executor > 0, ok
    return [m[:4] for m in ok]


@pytest.mark.parametrize("np_,signal", [(2, "stream"), (3, "stream"), (4, "stream"), (8, "stream"),
                                        (3, "host"), (1, "host")])
def test_collectv_check_p2p(np_, signal):
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal})
    ok = _all_ok(r, np_)
    if np_ > 1:
        assert {m for _, _, m, _ in ok} == {signal}, ok
        assert all(int(reads) > 0 for _, _, _, reads in ok), ok  # the kernels read peers' HBM


@pytest.mark.parametrize("np_", [2, 3])
def test_collectv_check_small_collect_off(np_):
    """SHMEMX_SMALL_COLLECT=0: lengths through the internal fcollect, every call on the
    executor, the same results."""
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_SMALL_COLLECT": "0"})
    _all_ok(r, np_, small_off=True)


@pytest.fixture
def no_leftover_messages():
    assert os.path.exists(FAKE), "tests/fakerccl/libsos_amd_fakerccl.so is not built"
    yield
    left = glob.glob("/dev/shm/fakerccl_*")
    for f in left:
        os.unlink(f)
    assert not left, f"unreceived messages: {left[:4]}"


@pytest.mark.parametrize("np_", [2, 3])
def test_collectv_check_rccl_executor(no_leftover_messages, np_):
    r = oshrun_fake(np_, PE_SCRIPT)
    _all_ok(r, np_)
    assert "fakerccl error" not in r.stderr, r.stderr[-2000:]
    sent = {int(rk): int(m) for rk, m in
            re.findall(r"fakerccl stats: rank (\d+) sent (\d+) messages", r.stderr)}
    assert sorted(sent) == list(range(np_)) and min(sent.values()) > 0, r.stderr[-2000:]


def test_collectv_check_rccl_native_allgather(no_leftover_messages, np_=2):
    """SHMEMX_RCCL_ALLGATHER=1: only a collect whose lengths are all equal may go to
    ncclAllGather; the uneven rounds stay send/receive pairs and every result holds."""
    r = oshrun_fake(np_, PE_SCRIPT, SHMEMX_RCCL_ALLGATHER="1")
    _all_ok(r, np_)
    assert "fakerccl error" not in r.stderr, r.stderr[-2000:]


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.mark.parametrize("np_", [2, 4])
def test_collect_ragged_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "collect_ragged")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"collect_ragged: OK ({np_} PEs)" in r.stdout
