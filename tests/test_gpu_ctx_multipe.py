"""GPU, several PE processes on one MI355X: the communication contexts through the public API
(tests/ctx_check_pe.py) over the p2p transport in both signalling modes and on a single PE;
two contexts sharing the one pool stream of SHMEMX_CTX_STREAMS=1; per-context completion read
from the library's own counters (the test build's sosx_ctx_stats); and the C example
examples/halo_ctx.c.  Helpers follow tests/test_gpu_rma_multipe.py.  No case provokes an
abort: the refusals are covered on the CPU by tests/test_ctx_checks.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSHRUN = os.path.join(ROOT, "tools", "oshrun")
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "ctx_check_pe.py")]
HOOKS_LIB = os.path.join(ROOT, "tests", "fakerccl", "libsos_amd_fakerccl.so")
# checks per PE, from the script's loops: 8 management, 16 cases x 8, p / g 5, atomics 10 + 3, put with
# signal 7 (a single PE has no team part)
FLOOR = 8 + 16 * 8 + 5 + 13 + 7


def oshrun(np_, cmd, timeout=240, extra_env=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M", "SHMEMX_STAGE_BYTES": "64M",
                "SHMEMX_DEVICE": "0", "SHMEMX_PUT_SIGNAL_FUSED_MAX": "1M", "PYTHONPATH": ROOT})
    env.update(extra_env or {})
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30), *cmd],
                          capture_output=True, text=True, timeout=timeout, env=env)


def pe_lines(r, np_, mode):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(rf"PE (\d+)/\d+: (\d+) {mode} checks OK \(p2p signal (\w+), context streams (\d+), "
                    r"peer reads (\d+), 0 unacquired\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    return ok


@pytest.mark.parametrize("np_,signal", [(1, "stream"), (2, "stream"), (3, "stream"), (2, "host")])
def test_each_family_through_a_context(np_, signal):
    """Every family through a created context against the same call on the default context,
    a team context, shmem_team_destroy delivering a pending put, shmem_finalize with a live
    context: results against numpy, canaries either side, 0 unacquired peer reads."""
    ok = pe_lines(oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal}), np_, "families")
    assert all(int(m[1]) >= FLOOR + (5 if np_ > 1 else 0) for m in ok), ok
    assert {m[3] for m in ok} == {"3"}, ok  # the default pool
    if np_ > 1:
        assert {m[2] for m in ok} == {signal}, ok
        assert all(int(m[4]) > 0 for m in ok), ok  # the gets and fetching atomics read peers' HBM


def test_two_contexts_share_one_pool_stream():
    """SHMEMX_CTX_STREAMS=1: both created contexts sit on the same stream; over-ordered, same results."""
    ok = pe_lines(oshrun(2, PE_SCRIPT, extra_env={"SHMEMX_CTX_STREAMS": "1"}), 2, "families")
    assert {m[3] for m in ok} == {"1"}, ok
    assert all(int(m[1]) >= FLOOR + 5 for m in ok), ok


def test_quiet_completes_its_own_context_alone():
    """Two contexts, a put_nbi on each: from the library's own counters, A and B sit on different
    streams, shmem_ctx_quiet(A) records no release on B and does not synchronise B's stream,
    shmem_quiet touches neither, and after shmem_ctx_quiet(B) both payloads are at the neighbour.
    The counters are the test build's (the library's twin with its hooks, here on the p2p
    transport, so its RCCL stand-in is never called)."""
    assert os.path.exists(HOOKS_LIB), "tests/fakerccl/libsos_amd_fakerccl.so is not built"
    ok = pe_lines(oshrun(2, PE_SCRIPT + ["completion"], extra_env={"SOSX_LIBRARY": HOOKS_LIB}), 2, "completion")
    assert all(int(m[1]) == 13 for m in ok), ok  # the expects of the script's completion mode


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "halo_ctx"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.mark.parametrize("np_", [2, 4])
def test_halo_ctx_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "halo_ctx")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"halo_ctx: OK ({np_} PEs)" in r.stdout
