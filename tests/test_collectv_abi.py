"""CPU: the shmem_collect surface: exported names and their pshmem_ twins, the generated
header, C11 and C++ programs that use the generic and the overloads, the Python mirrors,
and the argument checks of sosx_loopback_collect (it answers before any device work)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")


def exported_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3}


def gen():
    sys.path.insert(0, os.path.join(ROOT, "sos_amd", "csrc"))
    import gen_bindings
    return gen_bindings


def test_collectv_symbols_exported():
    g = gen()
    names = g.collectv_symbols()
    assert len(names) == 27 and len(set(names)) == 27
    assert sum(n.endswith("_collect") for n in names) == 24
    assert {"shmem_collectmem", "shmem_collect32", "shmem_collect64"} <= set(names)
    assert not set(names) & set(g.symbols()) and not set(names) & set(g.collect_symbols())
    exp = exported_symbols()
    missing = [n for n in names if n not in exp or "p" + n not in exp]
    assert not missing, missing
    for n in ("sosx_plan_encode_collect", "sosx_loopback_collect", "sos_api_collect",
              "sos_api_collect_active", "sosx_small_collect", "sosx_small_collect_calls"):
        assert n in exp, n


def test_collectv_header_functions_exported():
    text = open(os.path.join(INC, "shmem_collectv.h")).read()
    text = text.split("#if defined(__cplusplus)\nstatic inline")[0]  # skip inline overloads
    names = set()
    for m in re.finditer(r"^\s*(?:SHMEM_FUNCTION_ATTRIBUTES\s+)?[\w ]+?\**\s*\b(p?shmem_\w+)\(", text, re.M):
        names.add(m.group(1))
    assert len(names) == 54, len(names)  # (24 typed + mem + 2 active-set) x (shmem_, pshmem_)
    missing = sorted(names - exported_symbols())
    assert not missing, missing
    assert '#include "shmem_collectv.h"' in open(os.path.join(INC, "shmem.h")).read()


def test_generated_collectv_bindings_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sos_amd", "csrc", "gen_bindings.py"),
                        "--check"])
    assert r.returncode == 0
    src = open(os.path.join(ROOT, "sos_amd", "csrc", "collectv_gen.cpp")).read()
    assert 'sos_api_collect(team, dest, source, nelems, sizeof(long double), ' \
           '"shmem_longdouble_collect")' in src
    assert 'sos_api_collect_active(target, source, nlong, 8, PE_start, logPE_stride, PE_size, ' \
           'pSync, "shmem_collect64")' in src


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
def test_collectv_generics_compile_and_link(tmp_path, lang, ext):
    body = ('static long long a[16], b[16]; static double d[16], e[16]; static int i4[16], j4[16];\n'
            'static unsigned char u[16], v[16]; static long double x[16], y[16];\n'
            'static long ps[SHMEM_COLLECT_SYNC_SIZE];\n'
            'shmem_collect(SHMEM_TEAM_WORLD, a, b, 1); shmem_collect(SHMEM_TEAM_WORLD, d, e, 2);\n'
            'shmem_collect(SHMEM_TEAM_WORLD, i4, j4, 0); shmem_collect(SHMEM_TEAM_WORLD, u, v, 3);\n'
            'shmem_collect(SHMEM_TEAM_WORLD, x, y, 1);\n'
            'shmem_int_collect(SHMEM_TEAM_WORLD, i4, j4, 1); pshmem_int_collect(SHMEM_TEAM_WORLD, i4, j4, 1);\n'
            'shmem_collectmem(SHMEM_TEAM_WORLD, i4, j4, 4); pshmem_collectmem(SHMEM_TEAM_WORLD, i4, j4, 4);\n'
            'shmem_collect32(i4, j4, 1, 0, 0, shmem_n_pes(), ps);\n'
            'shmem_collect64(a, b, 1, 0, 0, shmem_n_pes(), ps);\n'
            'pshmem_collect64(a, b, 1, 0, 0, shmem_n_pes(), ps);\n')
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\nint main(void){ shmem_init();\n" + body +
                   "shmem_finalize(); return 0; }\n")
    _compile(str(src), lang, tmp_path)


def test_python_mirrors_exist():
    from sos_amd import _lib
    from sos_amd import shmem as S
    assert _lib.PLAN_COLLECT == 20
    for ty in ("int", "double", "uint8", "longdouble", "ptrdiff", "char"):
        fn = getattr(S, f"shmem_{ty}_collect")
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4
    assert len(S.shmem_collectmem.argtypes) == 4 and S.shmem_collectmem.restype is ctypes.c_int
    for bits in (32, 64):
        fn = getattr(S, f"shmem_collect{bits}")
        assert fn.restype is None and len(fn.argtypes) == 7
    assert callable(S.plan_collect) and callable(S.loopback_collect)
    # the older mirrors still resolve to their own functions
    assert S.shmem_int_fcollect is not None and len(S.shmem_int_alltoalls.argtypes) == 6


def test_loopback_collect_rejects_bad_args_without_gpu():
    from sos_amd import shmem as S
    L = S.lib()
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)  # host address: never dereferenced
    two = (ctypes.c_void_p * 2)(a, a + 64)
    nul = (ctypes.c_void_p * 2)(None, None)
    lens = (ctypes.c_size_t * 2)(4, 0)
    f = L.sosx_loopback_collect
    assert f(0, two, two, lens, None) == -3
    assert f(65, two, two, lens, None) == -3
    assert f(2, None, two, lens, None) == -3
    assert f(2, two, None, lens, None) == -3
    assert f(2, two, two, None, None) == -3
    assert f(2, nul, two, lens, None) == -3  # null source with a non-zero length
    assert f(2, two, nul, lens, None) == -3  # null target with a non-zero sum


def test_small_collect_counter_and_arg_checks_without_gpu():
    from sos_amd import _lib
    L = _lib.lib()
    assert L.sosx_small_collect_calls() == 0
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)  # host address: never dereferenced, nothing is launched
    one = (ctypes.c_void_p * 1)(a + 64)
    nul = (ctypes.c_void_p * 1)(None)
    n4 = (ctypes.c_size_t * 1)(4)
    nb = ctypes.c_int(0)
    f = L.sosx_small_collect
    assert f(a, one, n4, 0, a + 128, 1, ctypes.byref(nb), None) == -3
    assert f(a, one, n4, 65, a + 128, 1, ctypes.byref(nb), None) == -3
    assert f(a, nul, n4, 1, a + 128, 1, ctypes.byref(nb), None) == -3
    assert f(None, one, n4, 1, a + 128, 1, ctypes.byref(nb), None) == -3
