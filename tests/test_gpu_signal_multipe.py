"""GPU, several PE processes on one MI355X: put-with-signal, the signal operations and the
point-to-point waits and tests through the public API (tests/signal_check_pe.py) over the
p2p transport in both signalling modes and on a single PE, and the C example
examples/halo_signal.c.  Helpers follow tests/test_gpu_amo_multipe.py.  SHMEMX_P2P_TIMEOUT=30
bounds every wait, so a lost signal ends as an error message, not a hang.  No case provokes
an abort or a timeout: the refusals and the expiry message are CPU-side code
(tests/test_signal_checks.py)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSHRUN = os.path.join(ROOT, "tools", "oshrun")
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "signal_check_pe.py")]
# checks per PE, from the script's loops, on a single PE (more PEs: one more ping-pong phase).  put_signal: 60
# forms x 3 targets x (payload, signal) = 360; signal operations 6; the 202 wait / test forms once each, the
# name list, 4 empty / all-masked cases = 207; waits over one signal per PE 5; tests before / after 8; short
# ivars 2; host heap 5; ping-pong 4 sizes x (50 rounds x (signal, payload) + the final fetch) = 404; fused and
# composed both ran 1.
FLOOR = 360 + 6 + 207 + 5 + 8 + 2 + 5 + 404 + 1


def oshrun(np_, cmd, timeout=240, extra_env=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M", "SHMEMX_STAGE_BYTES": "64M",
                "SHMEMX_DEVICE": "0", "PYTHONPATH": ROOT, "SHMEMX_P2P_TIMEOUT": "30"})
    env.update(extra_env or {})
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30), *cmd],
                          capture_output=True, text=True, timeout=timeout, env=env)


@pytest.mark.parametrize("np_,signal", [(1, "stream"), (2, "stream"), (3, "stream"), (2, "host")])
def test_signal_check_p2p(np_, signal):
    # the limit is set here so that the ping-pong's sizes fall on both sides of it whatever the default is
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal, "SHMEMX_PUT_SIGNAL_FUSED_MAX": "1M"})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(r"PE (\d+)/\d+: (\d+) checks OK \(p2p signal (\w+), fused (\d+), composed (\d+), probes (\d+), "
                    r"0 unacquired\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    assert all(int(m[1]) >= FLOOR for m in ok), ok
    assert all(int(m[3]) > 0 and int(m[4]) > 0 and int(m[5]) > 0 for m in ok), ok
    if np_ > 1:
        assert {m[2] for m in ok} == {signal}, ok


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "halo_signal"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.mark.parametrize("np_", [2, 4])
def test_halo_signal_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "halo_signal")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"halo_signal: OK ({np_} PEs, 20 steps)" in r.stdout
