"""CPU: the fcollect / alltoall / alltoalls surface: exported names, the generated
header, C11 and C++ programs that use it, and the argument checks of sosx_strided_copy
and sosx_plan_extents (both answer before any device work)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")
REF_COLL = "/root/reference/src/collectives.c"
KINDS = ("fcollect", "alltoall", "alltoalls")


def exported_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3}


def gen():
    sys.path.insert(0, os.path.join(ROOT, "sos_amd", "csrc"))
    import gen_bindings
    return gen_bindings


def test_collect_symbols_exported():
    g = gen()
    names = g.collect_symbols()
    assert len(names) == 72 and len(set(names)) == 72
    for k in KINDS:
        assert sum(n.endswith("_" + k) for n in names) == 24
    assert len(g.symbols()) == 274 and not set(names) & set(g.symbols())
    names = names + [f"shmem_{k}mem" for k in KINDS] + [f"shmem_{k}{b}" for k in KINDS for b in (32, 64)]
    assert len(names) == 81
    exp = exported_symbols()
    missing = [n for n in names if n not in exp or "p" + n not in exp]
    assert not missing, missing


def test_collects_header_functions_exported():
    text = open(os.path.join(INC, "shmem_collects.h")).read()
    text = text.split("#if defined(__cplusplus)\nstatic inline")[0]  # skip inline overloads
    names = set()
    for m in re.finditer(r"^\s*(?:SHMEM_FUNCTION_ATTRIBUTES\s+)?[\w ]+?\**\s*\b(p?shmem_\w+)\(", text, re.M):
        names.add(m.group(1))
    assert len(names) == 162, len(names)  # (72 typed + 3 mem + 6 active-set) x (shmem_, pshmem_)
    missing = sorted(names - exported_symbols())
    assert not missing, missing
    assert '#include "shmem_collects.h"' in open(os.path.join(INC, "shmem.h")).read()


def test_generated_collect_bindings_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sos_amd", "csrc", "gen_bindings.py"),
                        "--check"])
    assert r.returncode == 0
    src = open(os.path.join(ROOT, "sos_amd", "csrc", "collects_gen.cpp")).read()
    assert 'sos_api_alltoalls(team, dest, source, dst, sst, nelems, sizeof(long double), ' \
           '"shmem_longdouble_alltoalls")' in src


def _compile(src, lang, tmp_path):
    exe = str(tmp_path / "a.out")
    cc = "gcc" if lang == "c" else "g++"
    std = ["-std=gnu11"] if lang == "c" else ["-std=c++17"]
    cmd = [cc, *std, "-Wall", "-Werror", "-I", INC, src, "-o", exe, "-L", os.path.dirname(LIB),
           "-lsos_amd", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("lang,ext", [("c", "c"), ("cxx", "cpp")])
def test_collect_generics_compile_and_link(tmp_path, lang, ext):
    body = ('static long long a[16], b[16]; static double d[16], e[16]; static int i4[16], j4[16];\n'
            'static long ps[SHMEM_ALLTOALLS_SYNC_SIZE];\n'
            'shmem_fcollect(SHMEM_TEAM_WORLD, a, b, 1); shmem_fcollect(SHMEM_TEAM_WORLD, d, e, 1);\n'
            'shmem_fcollect(SHMEM_TEAM_WORLD, i4, j4, 1);\n'
            'shmem_alltoall(SHMEM_TEAM_WORLD, a, b, 1); shmem_alltoall(SHMEM_TEAM_WORLD, d, e, 1);\n'
            'shmem_alltoall(SHMEM_TEAM_WORLD, i4, j4, 1);\n'
            'shmem_alltoalls(SHMEM_TEAM_WORLD, a, b, 2, 3, 1); shmem_alltoalls(SHMEM_TEAM_WORLD, d, e, 1, 2, 1);\n'
            'shmem_alltoalls(SHMEM_TEAM_WORLD, i4, j4, 2, 1, 1);\n'
            'shmem_fcollectmem(SHMEM_TEAM_WORLD, i4, j4, 4); shmem_alltoallmem(SHMEM_TEAM_WORLD, i4, j4, 4);\n'
            'shmem_alltoallsmem(SHMEM_TEAM_WORLD, i4, j4, 2, 2, 4);\n'
            'shmem_alltoalls64(a, b, 2, 3, 1, 0, 0, shmem_n_pes(), ps);\n')
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\nint main(void){ shmem_init();\n" + body +
                   "shmem_finalize(); return 0; }\n")
    _compile(str(src), lang, tmp_path)


def test_strided_copy_rejects_bad_args_without_gpu():
    from sos_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 63) & ~63  # 64-B aligned host address: never dereferenced
    f = L.sosx_strided_copy
    for es in (0, 3, 32):
        assert f(a, 1, a + 64, 2, es, 1, None) == -3, es
    for bad in (0, -1):
        assert f(a, bad, a + 64, 2, 4, 1, None) == -3
        assert f(a, 2, a + 64, bad, 4, 1, None) == -3
    assert f(None, 1, a, 2, 4, 1, None) == -3  # null pointer with count 1
    assert f(a, 1, None, 2, 4, 1, None) == -3
    assert f(a + 2, 1, a + 64, 2, 4, 1, None) == -3  # misaligned for the element size
    assert f(a, 1, a + 65, 2, 2, 1, None) == -3
    assert f(a, 1, a + 72, 2, 16, 1, None) == -3
    # count 0: nothing to do, whatever the pointers
    assert f(None, 1, None, 2, 4, 0, None) == 0
    assert f(a, 3, a + 64, 1, 16, 0, None) == 0


def test_plan_extents():
    from sos_amd import _lib
    L = _lib.lib()
    assert _lib.PLAN_FCOLLECT == 18 and _lib.PLAN_ALLTOALL == 19
    for P, n, ts in ((1, 1, 1), (3, 7, 4), (8, 4099, 16), (64, 5, 8)):
        assert _lib.plan_extents("fcollect", P, n, ts) == (n * ts, P * n * ts)
        assert _lib.plan_extents("alltoall", P, n, ts) == (P * n * ts, P * n * ts)
        assert _lib.plan_extents("ring", P, n, ts) == (n * ts, n * ts)
        assert _lib.plan_extents("inscan", P, n, ts) == (n * ts, n * ts)
        assert _lib.plan_extents(_lib.plan_bcast(0, True), P, n, ts) == (n * ts, n * ts)
    s, d = ctypes.c_ulonglong(7), ctypes.c_ulonglong(7)
    assert L.sosx_plan_extents(9, 4, 10, 4, ctypes.byref(s), ctypes.byref(d)) == -3  # no plan 9
    assert (s.value, d.value) == (7, 7)
    assert L.sosx_plan_extents(18, 0, 10, 4, ctypes.byref(s), ctypes.byref(d)) == -3
    assert L.sosx_plan_extents(19, 4, 10, 0, ctypes.byref(s), ctypes.byref(d)) == -3
    assert L.sosx_plan_extents(19, 4, 1 << 62, 4, ctypes.byref(s), ctypes.byref(d)) == -3  # overflow
    assert L.sosx_plan_extents(18, 4, 10, 4, None, None) == 0


@pytest.mark.skipif(not os.path.exists(REF_COLL), reason="reference checkout not present")
def test_reference_index_expressions_unchanged():
    """The closed forms of the collect tests restate these index expressions of SOS."""
    text = open(REF_COLL).read()
    for expr in ("my_as_rank * len", "peer_as_rank * len", "my_as_rank * nelems * dst * elem_size",
                 "peer_as_rank * nelems * sst * elem_size"):
        assert expr in text, expr
