"""GPU, several PE processes on one MI355X: the distributed locks through the public API
(tests/lock_check_pe.py) over the p2p transport in both signalling modes and on a single PE,
single-PE locks in static data and the host heap (tests/lock_static_pe.c, data segment
registered and pageable), and the C example examples/lock_counter.c.  Helpers follow
tests/test_gpu_signal_multipe.py.  SHMEMX_P2P_TIMEOUT=30 bounds every wait, so a lost hand-off
ends as an error message, not a hang.  No case provokes an abort or a timeout: the refusals,
the expiry message and the corrupt-word message are CPU-side code (tests/test_lock_checks.py)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSHRUN = os.path.join(ROOT, "tools", "oshrun")
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "lock_check_pe.py")]
K, TRIES = 25, 10


def floor(np_):
    """Checks per PE, from the script's loops: one per critical section (K through set_lock, TRIES
    through test_lock); the final counter, the unwritten log slots, one count per PE, this PE's lock
    word; test_lock once as the holder and once per other holder (a single PE: twice as the holder);
    this PE's lock word at the end."""
    return (K + TRIES) + 1 + 1 + np_ + 1 + (np_ if np_ > 1 else 2) + 1


def oshrun(np_, cmd, timeout=240, extra_env=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M", "SHMEMX_STAGE_BYTES": "64M",
                "SHMEMX_DEVICE": "0", "PYTHONPATH": ROOT, "SHMEMX_P2P_TIMEOUT": "30"})
    env.update(extra_env or {})
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30), *cmd],
                          capture_output=True, text=True, timeout=timeout, env=env)


@pytest.mark.parametrize("np_,signal", [(1, "stream"), (2, "stream"), (3, "stream"), (4, "stream"), (2, "host")])
def test_lock_check_p2p(np_, signal):
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(r"PE (\d+)/\d+: (\d+) checks OK \(lock launches (\d+), probes (\d+), 0 unacquired\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    assert all(int(m[1]) >= floor(np_) for m in ok), (ok, floor(np_))
    # at least one launch per set_lock (K), per successful test_lock (TRIES) and per clear_lock (K + TRIES)
    assert all(int(m[2]) >= 2 * (K + TRIES) for m in ok), ok


@pytest.fixture(scope="module")
def static_pe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lock_static") / "lock_static_pe")
    lib = os.path.join(ROOT, "sos_amd")
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "lock_static_pe.c"), "-o", exe, "-L", lib, "-lsos_amd",
                        f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("register", ["1", "0"])
def test_single_pe_locks_in_static_data_and_host_heap(static_pe, register):
    """SHMEMX_REGISTER_DATA=0 leaves the data segment pageable: no kernel may be handed it, the
    library completes its stream and the host runs the lock's steps."""
    r = oshrun(1, [static_pe], timeout=180, extra_env={"SHMEMX_REGISTER_DATA": register})
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    ok = re.findall(r"lock_static: PE 0/1 OK \((\d+) checks, data segment (\w+)\)", r.stdout)
    # per region: the fresh word, 5 set rounds x 3, 5 test rounds x 2, the counter = 27
    assert len(ok) == 1 and int(ok[0][0]) == 54, r.stdout + r.stderr[-2000:]
    if register == "0":
        assert ok[0][1] == "pageable", ok


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "lock_counter"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.mark.parametrize("np_", [2, 4])
def test_lock_counter_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "lock_counter")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"lock_counter: OK ({np_} PEs, 20 rounds)" in r.stdout
