"""CPU: the one-sided put / get surface: every name exported with its pshmem_ twin (strong)
and shmem_ form (weak), the committed name list, the generated headers compiled as C11 and
C++ with each generic and overload used once, the Python mirrors, and -- where the
reference tree is present -- the generated prototypes against its m4 tables."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rma_symbols.txt")
REF = "/root/reference"


def symbol_kinds():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    return {ln.split()[2]: ln.split()[1] for ln in out.splitlines() if len(ln.split()) == 3}


def gen():
    sys.path.insert(0, os.path.join(ROOT, "sos_amd", "csrc"))
    import gen_bindings
    return gen_bindings


def golden_names():
    return open(GOLDEN).read().split()


def test_name_list_is_the_generators():
    names = golden_names()
    assert len(names) == 285 and len(set(names)) == 285
    assert sorted(gen().rma_symbols()) == names
    # 24 types x (put, get, put_nbi, get_nbi, p, g, iput, iget) + ibput, ibget
    assert sum(bool(re.fullmatch(r"shmem_[a-z0-9]+_(put|get|put_nbi|get_nbi|p|g|iput|iget)", n)) for n in names) == 192
    assert sum(bool(re.fullmatch(r"shmemx_[a-z0-9]+_ib(put|get)", n)) for n in names) == 48
    for n in ("shmem_put8", "shmem_get128_nbi", "shmem_iput16", "shmem_iget64", "shmemx_ibput32",
              "shmemx_ibget128", "shmem_putmem", "shmem_getmem", "shmem_putmem_nbi", "shmem_getmem_nbi",
              "shmem_ptr", "shmem_longdouble_g", "shmem_ptrdiff_iput", "shmem_size_put_nbi"):
        assert n in names, n


def test_rma_symbols_exported_strong_and_weak():
    kinds = symbol_kinds()
    wrong = [n for n in golden_names()
             if kinds.get("p" + n) != "T" or kinds.get(n) != "W"]
    assert not wrong, wrong[:10]
    for n in ("sos_api_put", "sos_api_get", "sos_api_iput", "sos_api_iget", "sos_api_ibput", "sos_api_ibget",
              "sos_api_p", "sos_api_g", "sos_api_ptr", "sos_rma_check", "sosx_block_strided_copy",
              "sosx_block_copy_plan"):
        assert kinds.get(n) == "T", n


def test_headers_declare_exactly_the_names():
    names = set()
    for h in ("shmem_rma.h", "shmemx_rma.h"):
        text = open(os.path.join(INC, h)).read().split("#if defined(__cplusplus)\nstatic inline")[0]
        for m in re.finditer(r"^(?:SHMEM_FUNCTION_ATTRIBUTES\s+)?[\w ]+?\**\s*\b(p?shmemx?_\w+)\(", text, re.M):
            names.add(m.group(1))
    want = set(golden_names()) | {"p" + n for n in golden_names()}
    assert names == want, sorted(names ^ want)[:10]
    assert '#include "shmem_rma.h"' in open(os.path.join(INC, "shmem.h")).read()
    assert '#include "shmemx_rma.h"' in open(os.path.join(INC, "shmemx.h")).read()


def test_generated_rma_bindings_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sos_amd", "csrc", "gen_bindings.py"), "--check"])
    assert r.returncode == 0
    src = open(os.path.join(ROOT, "sos_amd", "csrc", "rma_gen.cpp")).read()
    assert 'sos_api_put(target, source, nelems, sizeof(long double), pe, 1, "shmem_longdouble_put_nbi");' in src
    assert 'sos_api_ibget(target, source, tst, sst, bsize, nblocks, 16, pe, "shmemx_ibget128");' in src
    assert 'sos_api_get(target, source, nelems, 1, pe, 0, "shmem_getmem");' in src


USES = '''static long a[16], b[16]; static double d[16], e[16]; static char c[16], f[16];
static long double x[4], y[4]; static unsigned short us[8], ut[8];
shmem_put(a, b, 1, 0); shmem_get(d, e, 2, 0); shmem_put_nbi(c, f, 3, 0); shmem_get_nbi(x, y, 1, 0);
shmem_p(a, 5L, 0); long v = shmem_g(a, 0); const double *ce = e; double w = shmem_g(ce, 0);
shmem_iput(us, ut, 2, 1, 3, 0); shmem_iget(d, e, 1, 2, 3, 0);
shmemx_ibput(a, b, 4, 4, 2, 2, 0); shmemx_ibget(d, e, 4, 4, 2, 2, 0);
shmem_put64(a, b, 1, 0); shmem_get8(c, f, 1, 0); shmem_put32_nbi(a, b, 1, 0); shmem_get16_nbi(us, ut, 1, 0);
shmem_iput128(x, y, 1, 1, 1, 0); shmem_iget64(a, b, 1, 1, 1, 0);
shmem_putmem(a, b, 8, 0); shmem_getmem(a, b, 8, 0); shmem_putmem_nbi(a, b, 8, 0); shmem_getmem_nbi(a, b, 8, 0);
shmemx_ibput32(a, b, 4, 4, 2, 2, 0); shmemx_ibget128(x, y, 1, 1, 1, 1, 0);
shmem_size_put((size_t *)a, (const size_t *)b, 1, 0); shmem_ptrdiff_p((ptrdiff_t *)a, 1, 0);
pshmem_long_put(a, b, 1, 0); pshmemx_long_ibget(a, b, 4, 4, 2, 2, 0); long double ld = pshmem_longdouble_g(x, 0);
void *p = shmem_ptr(a, 0); void *q = pshmem_ptr(a, 0); (void)p; (void)q; (void)v; (void)w; (void)ld;
'''


@pytest.mark.parametrize("lang,ext", [("c", "c"), ("cxx", "cpp")])
def test_rma_generics_compile_and_link(tmp_path, lang, ext):
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\n#include <shmemx.h>\nint main(void){ shmem_init();\n" + USES +
                   "shmem_finalize(); return 0; }\n")
    cc = "gcc" if lang == "c" else "g++"
    std = ["-std=c11"] if lang == "c" else ["-std=c++17"]
    cmd = [cc, *std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(tmp_path / "a.out"), "-L",
           os.path.dirname(LIB), "-lsos_amd", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_python_mirrors_exist():
    from sos_amd import _lib
    from sos_amd import shmem as S
    assert len(S.shmem_float_put.argtypes) == 4 and S.shmem_float_put.restype is None
    assert len(S.shmem_double_iget.argtypes) == 6 and len(S.shmemx_longdouble_ibput.argtypes) == 7
    assert S.shmem_longdouble_g.restype is ctypes.c_longdouble and len(S.shmem_short_p.argtypes) == 3
    assert len(S.shmem_getmem_nbi.argtypes) == 4 and len(S.shmemx_ibget64.argtypes) == 7
    for n, k in (("sos_api_put", 7), ("sos_api_get", 7), ("sos_api_iput", 8), ("sos_api_iget", 8),
                 ("sos_api_ibput", 9), ("sos_api_ibget", 9), ("sos_api_p", 5), ("sos_api_g", 5),
                 ("sos_api_ptr", 2), ("shmem_ptr", 2), ("sosx_block_strided_copy", 8)):
        assert len(getattr(S, n).argtypes) == k, n
    assert callable(_lib.block_strided_copy)
    # the older mirrors still resolve to their own functions
    assert len(S.shmem_int_alltoalls.argtypes) == 6 and len(S.shmem_float_sum_reduce.argtypes) == 4


def test_block_copy_rejects_bad_args_without_gpu():
    from sos_amd import shmem as S
    f = S.lib().sosx_block_strided_copy
    a = 1 << 20  # never dereferenced: every argument is checked before any device work
    assert f(a, 4, 2 * a, 4, 4, 2, 3, None) == -3      # element size
    assert f(a, 3, 2 * a, 4, 4, 2, 4, None) == -3      # stride < bsize
    assert f(None, 4, 2 * a, 4, 4, 2, 4, None) == -3   # null target
    assert f(a + 2, 4, 2 * a, 4, 4, 2, 4, None) == -3  # misaligned target
    assert f(None, 4, None, 4, 0, 2, 4, None) == 0     # nothing to move


def _m4_args(text):
    """Parameter types of an m4 prototype body: names dropped, $2 kept."""
    args = [re.sub(r"\s+", " ", a.strip()) for a in text.split(",")]
    return [re.sub(r"\s*\b\w+$", "", a).replace(" *", "*").replace("* ", "*").strip() for a in args]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present")
def test_prototypes_match_the_reference_tables():
    """Every generated prototype against the reference's m4 declaration of the same form:
    return type and parameter types, for the typed ($1/$2) and the sized forms."""
    g = gen()
    decls = {}
    for path in ("mpp/shmem_c_func.h4", "mpp/shmemx_c_func.h4"):
        text = re.sub(r"SH_PAD\(`\$1'\)", "", open(os.path.join(REF, path)).read())
        for m in re.finditer(r"SHMEM_FUNCTION_ATTRIBUTES\s+([\w$ ]+?\*?)\s*SHPRE\(\)(shmemx?_[\w$]+)\(([^)]*)\)", text):
            ret, name, args = m.groups()
            decls[name] = (ret.strip(), _m4_args(args))
    # the type table itself
    bind = open(os.path.join(REF, "bindings/shmem_bind_c.m4")).read()
    table = bind.split("define(`SHMEM_BIND_C_RMA'")[1].split("')dnl")[0]
    ref_types = re.findall(r"\$1\((\w+),\s*([\w ]+?)\)", table)
    assert ref_types == list(g.RMA), ref_types[:3]
    sizes = bind.split("define(`SHMEM_BIND_C_SIZES'")[1].split("')dnl")[0]
    assert [int(b) for b, _ in re.findall(r"\$1\((\d+),\s*(\d+)\)", sizes)] == list(g.RMA_SIZES)
    checked = 0
    for hdr, name, sig, _ in g.rma_entries():
        proto = sig("")
        ret, rest = proto.split(name + "(")
        mine = _m4_args(rest.rstrip(")"))
        m = re.fullmatch(r"(shmemx?)_([a-z0-9]+)_(\w+)", name)
        cands = []
        if m and (m.group(2), ) in {(s,) for s, _ in g.RMA}:
            ct = dict(g.RMA)[m.group(2)]
            cands.append((f"{m.group(1)}_$1_{m.group(3)}", ct))
        m2 = re.fullmatch(r"(shmemx?_[a-z]+?)(\d+|mem)(_nbi)?", name)
        if m2:
            cands.append((f"{m2.group(1)}$1{m2.group(3) or ''}", None))
        cands.append((name, None))
        for key, ct in cands:
            if key in decls:
                rret, rargs = decls[key]
                if ct:
                    rret = rret.replace("$2", ct)
                    rargs = [a.replace("$2", ct) for a in rargs]
                assert ret.strip() == rret, (name, ret, rret)
                assert mine == rargs, (name, mine, rargs)
                checked += 1
                break
        else:
            raise AssertionError(f"{name}: no declaration in the reference")
    assert checked == 284
    assert decls["shmem_ptr"] == ("void *", ["const void*", "int"]) or decls["shmem_ptr"][1] == ["const void*", "int"]
