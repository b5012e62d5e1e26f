"""GPU, several PE processes on one MI355X: the atomic memory operations through the public
API (tests/amo_check_pe.py) over the p2p transport in both signalling modes and on a single
PE, the self-PE forms on static data and the host heap (tests/amo_static_pe.c, data
segment registered and pageable), and the C example examples/ticket_counter.c.  Helpers
follow tests/test_gpu_rma_multipe.py.  No case provokes an abort: the refusals are covered
on the CPU by tests/test_amo_checks.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSHRUN = os.path.join(ROOT, "tools", "oshrun")
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "amo_check_pe.py")]
# checks per PE, from the script's loops.  Integer forms, 3 targets each, one check of the old value per
# fetching form and one of the final word per form: int and size 3 x (8 + 11) = 57 each, long 57 + the
# deprecated names' 3 x (5 + 8) = 96, uint64 57 + the bitwise forms' 3 x (3 + 6) = 84, uint32 27;
# float and double 3 x (6 + 8) + 8 raw words = 50 each; contended counter 3, burst 1, claim word 3;
# nbi forms 9 per kind of `fetch` memory x 3; host-heap targets 7.
FLOOR = 321 + 100 + 7 + 27 + 7


def oshrun(np_, cmd, timeout=240, extra_env=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M", "SHMEMX_STAGE_BYTES": "64M",
                "SHMEMX_DEVICE": "0", "PYTHONPATH": ROOT})
    env.update(extra_env or {})
    return subprocess.run([sys.executable, OSHRUN, "-np", str(np_), "--timeout", str(timeout - 30), *cmd],
                          capture_output=True, text=True, timeout=timeout, env=env)


@pytest.mark.parametrize("np_,signal", [(1, "stream"), (2, "stream"), (3, "stream"), (2, "host")])
def test_amo_check_p2p(np_, signal):
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(r"PE (\d+)/\d+: (\d+) checks OK \(p2p signal (\w+), peer reads (\d+), 0 unacquired\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    assert all(int(m[1]) >= FLOOR for m in ok), ok
    if np_ > 1:
        assert {m[2] for m in ok} == {signal}, ok
        assert all(int(m[3]) > 0 for m in ok), ok  # the fetching forms on a peer's word read its HBM


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "ticket_counter"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.fixture(scope="module")
def static_pe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("amo_static") / "amo_static_pe")
    lib = os.path.join(ROOT, "sos_amd")
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "amo_static_pe.c"), "-o", exe, "-L", lib, "-lsos_amd",
                        f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("np_,register", [(1, "1"), (2, "1"), (1, "0"), (2, "0")])
def test_self_pe_targets_in_static_data_and_host_heap(static_pe, np_, register):
    """Every form with the calling PE as the target and the word in static data or the host
    heap.  SHMEMX_REGISTER_DATA=0 leaves the data segment pageable: no kernel may be handed
    it, the library completes its stream and the host does the operation."""
    r = oshrun(np_, [static_pe], timeout=180, extra_env={"SHMEMX_REGISTER_DATA": register})
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    ok = re.findall(r"amo_static: PE (\d+)/\d+ OK \((\d+) checks, data segment (\w+)\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout + r.stderr[-2000:]
    assert all(int(m[1]) == 54 for m in ok), ok  # 27 per region
    if register == "0":
        assert {m[2] for m in ok} == {"pageable"}, ok


@pytest.mark.parametrize("np_", [2, 4])
def test_ticket_counter_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "ticket_counter")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"ticket_counter: OK ({np_} PEs)" in r.stdout
