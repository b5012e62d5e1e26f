"""CPU: the atomic-memory-operation surface: every name exported with its pshmem_ twin
(strong) and shmem_ form (weak), the committed name list with its per-form counts, the
generated header compiled as C11 and C++ with each generic and overload used once, the
Python mirrors, and -- where the reference tree is present -- the generated prototypes
and type tables against its m4 sources."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "amo_symbols.txt")
REF = "/root/reference"

AMO_FORMS = ["atomic_compare_swap", "atomic_fetch_inc", "atomic_inc", "atomic_fetch_add", "atomic_add",
             "cswap", "finc", "inc", "fadd", "add",
             "atomic_compare_swap_nbi", "atomic_fetch_inc_nbi", "atomic_fetch_add_nbi"]
EXTENDED_FORMS = ["atomic_swap", "atomic_fetch", "atomic_set", "swap", "fetch", "set", "atomic_swap_nbi",
                  "atomic_fetch_nbi"]
BITWISE_FORMS = ["atomic_and", "atomic_or", "atomic_xor", "atomic_fetch_and", "atomic_fetch_or", "atomic_fetch_xor",
                 "atomic_fetch_and_nbi", "atomic_fetch_or_nbi", "atomic_fetch_xor_nbi"]
DEPRECATED = ("cswap", "finc", "inc", "fadd", "add", "swap", "fetch", "set")


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
    g = gen()
    names = golden_names()
    want = (len(g.AMO) * len(AMO_FORMS) + len(g.EXTENDED_AMO) * len(EXTENDED_FORMS)
            + len(g.BITWISE_AMO) * len(BITWISE_FORMS))
    assert (len(g.AMO), len(g.EXTENDED_AMO), len(g.BITWISE_AMO)) == (12, 14, 7)
    assert len(names) == want == 331 and len(set(names)) == want
    assert sorted(g.amo_symbols()) == names
    # every form over exactly its table's types
    for forms, table in ((AMO_FORMS, g.AMO), (EXTENDED_FORMS, g.EXTENDED_AMO), (BITWISE_FORMS, g.BITWISE_AMO)):
        for form in forms:
            have = sorted(n for n in names if any(n == f"shmem_{st}_{form}" for st, _ in g.EXTENDED_AMO))
            assert have == sorted(f"shmem_{st}_{form}" for st, _ in table), form
    for n in ("shmem_float_atomic_swap", "shmem_double_atomic_fetch_nbi", "shmem_ptrdiff_atomic_compare_swap_nbi",
              "shmem_size_finc", "shmem_uint32_atomic_fetch_xor_nbi", "shmem_int64_atomic_and"):
        assert n in names, n
    for n in ("shmem_float_atomic_add", "shmem_int_atomic_and", "shmem_long_atomic_fetch_or", "shmem_double_atomic_inc",
              "shmem_size_atomic_xor", "shmem_short_atomic_add"):
        assert n not in names, n
    # the one-sided list is not touched
    assert not set(names) & set(g.rma_symbols())


def test_amo_symbols_exported_strong_and_weak():
    kinds = symbol_kinds()
    wrong = [n for n in golden_names() if kinds.get("p" + n) != "T" or kinds.get(n) != "W"]
    assert not wrong, wrong[:10]
    for n in ("sos_api_amo", "sos_amo_check", "sosx_amo"):
        assert kinds.get(n) == "T", n
    assert not [n for n in kinds if "shmem_ctx_" in n]


def test_header_declares_exactly_the_names():
    text = open(os.path.join(INC, "shmem_amo.h")).read().split("#if defined(__cplusplus)\nstatic inline")[0]
    names, deprecated = set(), set()
    for m in re.finditer(r"^(?:SHMEM_FUNCTION_ATTRIBUTES\s+)?[\w ]+?\**\s*\b(p?shmem_\w+)\(([^)]*)\)([^;]*);", text, re.M):
        names.add(m.group(1))
        if "SHMEM_ATTRIBUTE_DEPRECATED" in m.group(3):
            deprecated.add(m.group(1))
    want = set(golden_names()) | {"p" + n for n in golden_names()}
    assert names == want, sorted(names ^ want)[:10]
    old = {n for n in want if re.fullmatch(r"p?shmem_[a-z0-9]+_(%s)" % "|".join(DEPRECATED), n)}
    assert deprecated == old and len(old) == 2 * (12 * 5 + 14 * 3)
    assert "#define SHMEM_ATTRIBUTE_DEPRECATED __attribute__((deprecated))" in text
    assert '#include "shmem_amo.h"' in open(os.path.join(INC, "shmem.h")).read()
    # nothing of this went into the one-sided headers
    for h in ("shmem_rma.h", "shmemx_rma.h"):
        assert "atomic" not in open(os.path.join(INC, h)).read()


def test_generated_amo_bindings_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sos_amd", "csrc", "gen_bindings.py"), "--check"])
    assert r.returncode == 0
    src = open(os.path.join(ROOT, "sos_amd", "csrc", "amo_gen.cpp")).read()
    assert ('long old; sos_api_amo(SOSX_AMO_ADD, target, &value, NULL, &old, 1, sizeof(long), 0, pe, 0, '
            '"shmem_long_atomic_fetch_add"); return old;') in src
    assert ('int value = 1; sos_api_amo(SOSX_AMO_ADD, target, &value, NULL, NULL, 0, sizeof(int), 0, pe, 0, '
            '"shmem_int_atomic_inc");') in src
    assert ('sos_api_amo(SOSX_AMO_SWAP, target, &value, NULL, fetch, 1, sizeof(float), 1, pe, 1, '
            '"shmem_float_atomic_swap_nbi");') in src
    assert ('sos_api_amo(SOSX_AMO_CSWAP, target, &value, &cond, &old, 1, sizeof(uint64_t), 0, pe, 0, '
            '"shmem_uint64_cswap");') in src
    # the two new files are what the generator writes (and so what --check compares)
    assert open(os.path.join(INC, "shmem_amo.h")).read() == gen().amo_header()
    assert src == gen().amo_source()


# each generic / overload once; the arms differ by table (bitwise: no signed base type in C++)
USES_NEW = '''static int i; static long l; static long long ll; static unsigned u; static unsigned long ul;
static unsigned long long ull; static float f; static double d; static const double cd = 1.0;
static int fi; static long fl; static float ff; static double fd; static unsigned fu; static unsigned long ful;
i = shmem_atomic_compare_swap(&i, 0, 1, 0); l = shmem_atomic_fetch_inc(&l, 0); shmem_atomic_inc(&ll, 0);
u = shmem_atomic_fetch_add(&u, 2u, 0); shmem_atomic_add(&ul, 3ul, 0);
shmem_atomic_compare_swap_nbi(&fi, &i, 0, 1, 0); shmem_atomic_fetch_inc_nbi(&fl, &l, 0);
shmem_atomic_fetch_add_nbi(&fu, &u, 2u, 0);
f = shmem_atomic_swap(&f, 1.5f, 0); d = shmem_atomic_fetch(&d, 0); d = shmem_atomic_fetch(&cd, 0);
shmem_atomic_set(&ull, 4ull, 0); shmem_atomic_swap_nbi(&ff, &f, 2.5f, 0); shmem_atomic_fetch_nbi(&fd, &d, 0);
shmem_atomic_fetch_nbi(&fd, &cd, 0);
shmem_atomic_and(&u, 1u, 0); shmem_atomic_or(&ul, 1ul, 0); shmem_atomic_xor(&ull, 1ull, 0);
u = shmem_atomic_fetch_and(&u, 1u, 0); ul = shmem_atomic_fetch_or(&ul, 1ul, 0); ull = shmem_atomic_fetch_xor(&ull, 1ull, 0);
shmem_atomic_fetch_and_nbi(&fu, &u, 1u, 0); shmem_atomic_fetch_or_nbi(&ful, &ul, 1ul, 0);
shmem_atomic_fetch_xor_nbi(&fu, &u, 1u, 0);
static size_t sz; static ptrdiff_t pd; static uint32_t u32; static int64_t i64;
sz = shmem_size_atomic_fetch_add(&sz, 1, 0); pd = pshmem_ptrdiff_atomic_swap(&pd, 1, 0);
u32 = shmem_uint32_atomic_fetch_xor(&u32, 1, 0); shmem_int64_atomic_or(&i64, 1, 0);
pshmem_double_atomic_set(&d, 2.0, 0); i64 = pshmem_int64_atomic_fetch_and(&i64, 1, 0);
'''
USES_C11_ONLY = '''static int32_t i32; static int64_t j64; static int32_t fi32;
shmem_atomic_and(&i32, 1, 0); j64 = shmem_atomic_fetch_or(&j64, 1, 0); shmem_atomic_fetch_xor_nbi(&fi32, &i32, 1, 0);
'''
USES_OLD = '''static int i; static long l; static long long ll; static unsigned u; static float f; static double d;
i = shmem_cswap(&i, 0, 1, 0); l = shmem_finc(&l, 0); shmem_inc(&ll, 0); u = shmem_fadd(&u, 2u, 0); shmem_add(&l, 3l, 0);
f = shmem_swap(&f, 1.5f, 0); d = shmem_fetch(&d, 0); shmem_set(&i, 4, 0);
l = shmem_long_cswap(&l, 0, 1, 0); l = shmem_long_finc(&l, 0); shmem_long_inc(&l, 0); l = shmem_long_fadd(&l, 1, 0);
shmem_long_add(&l, 1, 0); d = shmem_double_swap(&d, 1.0, 0); f = shmem_float_fetch(&f, 0); shmem_size_set((size_t *)&l, 1, 0);
'''


def _build(tmp_path, lang, body, flags=()):
    ext = "c" if lang == "c" else "cpp"
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\n#include <shmemx.h>\nint main(void){ shmem_init();\n" + body +
                   "shmem_finalize(); return 0; }\n")
    cc = "gcc" if lang == "c" else "g++"
    std = ["-std=c11"] if lang == "c" else ["-std=c++17"]
    cmd = [cc, *std, "-Wall", "-Werror", *flags, "-I", INC, str(src), "-o", str(tmp_path / "a.out"), "-L",
           os.path.dirname(LIB), "-lsos_amd", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-L/opt/rocm/lib", "-lamdhip64"]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.parametrize("lang", ["c", "cxx"])
def test_amo_generics_compile_and_link(tmp_path, lang):
    r = _build(tmp_path, lang, USES_NEW + (USES_C11_ONLY if lang == "c" else ""))
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("lang", ["c", "cxx"])
def test_deprecated_names_compile_and_warn(tmp_path, lang):
    r = _build(tmp_path, lang, USES_OLD, flags=["-Wno-deprecated-declarations"])
    assert r.returncode == 0, r.stderr[-3000:]
    # without the flag the typed deprecated names are refused under -Werror
    r = _build(tmp_path, lang, "static long l; shmem_long_add(&l, 1, 0);\n")
    assert r.returncode != 0 and "deprecated" in r.stderr, r.stderr[-2000:]


def test_python_mirrors():
    from sos_amd import shmem as S
    c = ctypes
    f = S.shmem_long_atomic_fetch_add
    assert f.restype is c.c_long and f.argtypes == [c.c_void_p, c.c_long, c.c_int]
    f = S.shmem_int_atomic_compare_swap
    assert f.restype is c.c_int and f.argtypes == [c.c_void_p, c.c_int, c.c_int, c.c_int]
    f = S.shmem_float_atomic_swap
    assert f.restype is c.c_float and f.argtypes == [c.c_void_p, c.c_float, c.c_int]
    f = S.shmem_double_atomic_set
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_double, c.c_int]
    f = S.shmem_double_atomic_fetch
    assert f.restype is c.c_double and f.argtypes == [c.c_void_p, c.c_int]
    f = S.shmem_uint64_atomic_fetch_inc
    assert f.restype is c.c_uint64 and f.argtypes == [c.c_void_p, c.c_int]
    f = S.shmem_size_atomic_inc
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_int]
    f = S.shmem_uint32_atomic_fetch_or_nbi
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_void_p, c.c_uint32, c.c_int]
    f = S.shmem_ptrdiff_atomic_compare_swap_nbi
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_void_p, c.c_ssize_t, c.c_ssize_t, c.c_int]
    f = S.shmem_float_atomic_fetch_nbi
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_void_p, c.c_int]
    f = S.shmem_uint64_atomic_xor
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_uint64, c.c_int]
    # the deprecated names mirror their new forms
    for old, new in (("cswap", "atomic_compare_swap"), ("finc", "atomic_fetch_inc"), ("inc", "atomic_inc"),
                     ("fadd", "atomic_fetch_add"), ("add", "atomic_add"), ("swap", "atomic_swap"),
                     ("fetch", "atomic_fetch"), ("set", "atomic_set")):
        a, b = getattr(S, f"shmem_long_{old}"), getattr(S, f"shmem_long_{new}")
        assert a.restype is b.restype and a.argtypes == b.argtypes, old
    assert len(S.sos_api_amo.argtypes) == 11 and len(S.sosx_amo.argtypes) == 8 and len(S.sos_amo_check.argtypes) == 4
    # every generated name resolves, and the one-sided mirrors are still their own
    for n in golden_names():
        assert getattr(S, n).argtypes[-1] is c.c_int, n
    assert len(S.shmem_long_p.argtypes) == 3 and S.shmem_long_g.restype is c.c_long
    assert len(S.shmem_float_put.argtypes) == 4


def _m4_args(text):
    """Parameter types of an m4 prototype body: names dropped, $2 kept."""
    args = [re.sub(r"\s+", " ", a.strip()) for a in text.split(",")]
    return [re.sub(r"\s*\b\w+$", "", a).replace(" *", "*").replace("* ", "*").strip() for a in args]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present")
def test_prototypes_match_the_reference_tables():
    """Every generated prototype against the reference's m4 declaration of the same form
    (return type, parameter types, the deprecation mark), the three type tables against
    bindings/shmem_bind_c.m4, and the generic selectors' arms against the C11 and C++
    binding tables."""
    g = gen()
    text = re.sub(r"SH_PAD\(`\$1'\)", "", open(os.path.join(REF, "mpp/shmem_c_func.h4")).read())
    decls = {}
    for m in re.finditer(r"SHMEM_FUNCTION_ATTRIBUTES\s+([\w$ ]+?\*?)\s*SHPRE\(\)(shmem_\$1_\w+)\(([^)]*)\)([^'\n]*)", text):
        ret, name, args, tail = m.groups()
        decls[name] = (ret.strip(), _m4_args(args), "SHMEM_ATTRIBUTE_DEPRECATED" in tail)

    def table(path, macro):
        body = open(os.path.join(REF, path)).read().split(f"define(`{macro}'")[1].split("')dnl")[0]
        return re.findall(r"\$1\((\w+),\s*([\w ]+?),", body)

    ref_amo = table("bindings/shmem_bind_c.m4", "SHMEM_BIND_C_AMO")
    assert ref_amo == list(g.AMO)
    assert ref_amo + table("bindings/shmem_bind_c.m4", "SHMEM_BIND_C_EXTENDED_AMO") == list(g.EXTENDED_AMO)
    assert table("bindings/shmem_bind_c.m4", "SHMEM_BIND_C_BITWISE_AMO") == list(g.BITWISE_AMO)
    for lang, mine in (("c11", g.AMO_GENERIC_C11), ("cxx", g.AMO_GENERIC_CXX)):
        for key in ("AMO", "EXTENDED_AMO", "BITWISE_AMO"):
            assert table(f"bindings/shmem_bind_{lang}.m4", f"SHMEM_BIND_{lang.upper()}_{key}") == list(mine[key]), (lang, key)
    checked = 0
    header = open(os.path.join(INC, "shmem_amo.h")).read()
    for name, sig, _, dep in g.amo_entries():
        st, form = re.fullmatch(r"shmem_([a-z0-9]+?)_((?:atomic_)?\w+)", name).groups()
        ct = dict(g.EXTENDED_AMO)[st]
        rret, rargs, rdep = decls[f"shmem_$1_{form}"]
        ret, rest = sig("").split(name + "(")
        assert ret.strip() == rret.replace("$2", ct), (name, ret, rret)
        assert _m4_args(rest.rstrip(")")) == [a.replace("$2", ct) for a in rargs], name
        assert dep == rdep, name
        assert (f"{sig('')} SHMEM_ATTRIBUTE_DEPRECATED;" in header) == rdep, name
        checked += 1
    assert checked == 331
