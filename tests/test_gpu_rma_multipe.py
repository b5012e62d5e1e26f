"""GPU, several PE processes on one MI355X: the one-sided put / get family through the
public API (tests/rma_check_pe.py) over the p2p transport in both signalling modes and on
a single PE, the self-PE forms on static data and the host heap
(tests/rma_static_pe.c, data segment registered and pageable), and the C example
examples/halo_put.c.  Helpers follow
tests/test_gpu_collectv_multipe.py.  No case provokes an abort: the refusals are covered
on the CPU by tests/test_rma_checks.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSHRUN = os.path.join(ROOT, "tools", "oshrun")
PE_SCRIPT = [sys.executable, os.path.join(ROOT, "tests", "rma_check_pe.py")]
# checks per PE, from the script's loops: put/get 170 (float: 4 sizes x 3 local kinds x 2 PEs x 2, the
# other five types 4 x 1 x 2 x 2; per type 4 put_nbi, 1 get_nbi, 2 p/g), iput/iget 144, ibput/ibget 60,
# shmem_ptr 3 (+ 1 with a peer), reductions 3, self-PE forms on the host heap 54 (9 shapes x 3 local
# kinds x 2)
FLOOR = 434


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
def test_rma_check_p2p(np_, signal):
    r = oshrun(np_, PE_SCRIPT, extra_env={"SHMEMX_P2P_SIGNAL": signal})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ok = re.findall(r"PE (\d+)/\d+: (\d+) checks OK \(p2p signal (\w+), peer reads (\d+), 0 unacquired\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout[-3000:] + r.stderr[-3000:]
    assert all(int(m[1]) >= FLOOR for m in ok), ok
    if np_ > 1:
        assert {m[2] for m in ok} == {signal}, ok
        assert all(int(m[3]) > 0 for m in ok), ok  # gets and the reductions read peers' HBM


@pytest.fixture(scope="module")
def examples():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "halo_put"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return os.path.join(ROOT, "examples")


@pytest.fixture(scope="module")
def static_pe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rma_static") / "rma_static_pe")
    lib = os.path.join(ROOT, "sos_amd")
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "rma_static_pe.c"),
                        "-o", exe, "-L", lib, "-lsos_amd", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-lamdhip64"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("np_,register", [(1, "1"), (2, "1"), (1, "0"), (2, "0")])
def test_self_pe_forms_on_static_data_and_host_heap(static_pe, np_, register):
    """iput / iget / ibput / ibget / put / get with the calling PE as the target and the
    symmetric side in static data or the host heap, the local side in device, malloc and
    static memory.  SHMEMX_REGISTER_DATA=0 leaves the data segment pageable: no kernel may
    be handed it, the library stages it (or moves host-to-host blocks itself)."""
    r = oshrun(np_, [static_pe], timeout=180, extra_env={"SHMEMX_REGISTER_DATA": register})
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    ok = re.findall(r"rma_static: PE (\d+)/\d+ OK \((\d+) checks, data segment (\w+)\)", r.stdout)
    assert sorted(int(m[0]) for m in ok) == list(range(np_)), r.stdout + r.stderr[-2000:]
    assert all(int(m[1]) == 108 for m in ok), ok  # 3 local kinds x 2 regions x 18 (6 ibput, 2 iput, 1 put; as many gets)
    if register == "0":
        assert {m[2] for m in ok} == {"pageable"}, ok


@pytest.mark.parametrize("np_", [2, 4])
def test_halo_put_example(examples, np_):
    r = oshrun(np_, [os.path.join(examples, "halo_put")], timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert f"halo_put: OK ({np_} PEs)" in r.stdout
