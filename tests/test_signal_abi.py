"""CPU: the put-with-signal, signal and point-to-point synchronisation surface: every name
exported with its pshmem_ twin (strong) and shmem_ form (weak), the committed name list
equal to what the generator produces, the generated headers compiled as C11 and C++ with
each generic and overload used once, the deprecated waits warning, the constants with the
reference's values, and the Python mirrors."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "signal_symbols.txt")

SYNC_FORMS = [f"{w}{k}{v}" for w in ("wait_until", "test") for k, v in
              (("", ""), ("_all", ""), ("_any", ""), ("_some", ""), ("_all", "_vector"), ("_any", "_vector"), ("_some", "_vector"))]


def symbol_kinds():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
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
    assert (len(g.RMA), len(g.SYNC), len(g.WAIT), len(SYNC_FORMS)) == (24, 14, 4, 14)
    want = 2 * (24 + 5 + 1) + 4 + 14 * 14 + 4 + 2
    assert len(names) == want == 266 and len(set(names)) == want
    assert sorted(g.signal_symbols()) == names
    for form in SYNC_FORMS:
        assert sorted(n for n in names if re.fullmatch(rf"shmem_[a-z0-9]+_{form}", n) and n != "shmem_signal_wait_until") == \
            sorted(f"shmem_{st}_{form}" for st, _ in g.SYNC), form
    assert sorted(n for n in names if re.fullmatch(r"shmem_[a-z0-9]+_wait", n)) == \
        sorted(f"shmem_{st}_wait" for st, _ in g.WAIT)
    for sfx in ("", "_nbi"):
        assert sorted(n for n in names if re.fullmatch(rf"shmem_[a-z0-9]+_put_signal{sfx}", n)) == \
            sorted(f"shmem_{st}_put_signal{sfx}" for st, _ in g.RMA)
    for n in ("shmem_put8_signal", "shmem_put128_signal_nbi", "shmem_putmem_signal", "shmem_putmem_signal_nbi",
              "shmem_signal_fetch", "shmemx_signal_add", "shmemx_signal_set", "shmem_signal_wait_until",
              "shmem_wait", "shmem_wait_until", "shmem_ptrdiff_test_some_vector", "shmem_ushort_wait_until_any"):
        assert n in names, n
    for n in ("shmem_float_wait_until", "shmem_char_test", "shmem_ushort_wait", "shmem_put256_signal",
              "shmem_ctx_long_put_signal", "shmem_long_wait_vector", "shmem_long_test_vector"):
        assert n not in names, n
    assert not set(names) & (set(g.rma_symbols()) | set(g.amo_symbols()))


def test_symbols_exported_strong_and_weak():
    kinds = symbol_kinds()
    wrong = [n for n in golden_names() if kinds.get("p" + n) != "T" or kinds.get(n) != "W"]
    assert not wrong, wrong[:10]
    for n in ("sos_api_put_signal", "sos_api_signal_op", "sos_api_signal_fetch", "sos_api_wait", "sos_api_test",
              "sos_put_signal_check", "sos_sync_check", "sos_sync_eval", "sosx_put_signal", "sosx_sync_snapshot",
              "sosx_put_signal_plan"):
        assert kinds.get(n) == "T", n
    assert not [n for n in kinds if "shmem_ctx_" in n]


def test_headers_declare_exactly_the_names():
    names, deprecated, guarded = set(), set(), set()
    for h in ("shmem_signal.h", "shmem_sync.h"):
        text = open(os.path.join(INC, h)).read().split("#if defined(__cplusplus)\nstatic inline")[0]
        for m in re.finditer(r"^(?:SHMEM_FUNCTION_ATTRIBUTES\s+)?[\w ]+?\**\s*\b(p?shmemx?_\w+)\(([^)]*)\)([^;]*);", text, re.M):
            names.add(m.group(1))
            if "SHMEM_ATTRIBUTE_DEPRECATED" in m.group(3):
                deprecated.add(m.group(1))
        guarded |= set(re.findall(r"#if \(!defined\(__cplusplus\)[^\n]*\n[^\n]*?\b(p?shmem_\w+)\(", text))
    want = set(golden_names()) | {"p" + n for n in golden_names()}
    assert names == want, sorted(names ^ want)[:10]
    assert deprecated == {p + f"shmem_{st}wait" for p in ("", "p") for st in ("short_", "int_", "long_", "longlong_", "")}
    # the untyped wait_until is declared where the reference declares it: not under the generics
    assert guarded == {"shmem_wait_until", "pshmem_wait_until"}
    shmem_h = open(os.path.join(INC, "shmem.h")).read()
    assert '#include "shmem_signal.h"' in shmem_h and '#include "shmem_sync.h"' in shmem_h


def test_generated_bindings_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sos_amd", "csrc", "gen_bindings.py"), "--check"])
    assert r.returncode == 0
    g = gen()
    src = open(os.path.join(ROOT, "sos_amd", "csrc", "signal_gen.cpp")).read()
    assert src == g.signal_source()
    assert open(os.path.join(INC, "shmem_signal.h")).read() == g.signal_header("signal")
    assert open(os.path.join(INC, "shmem_sync.h")).read() == g.signal_header("sync")
    # one line per entry point: its family's macro over (name, C type, ...), or SOS_ENTRY itself
    lines = src.split("\n")
    for want in ("SOS_PUT_SIGNAL(shmem_longdouble_put_signal_nbi, long double, sizeof(long double), 1)",
                 "SOS_PUT_SIGNAL(shmem_put128_signal, void, 16, 0)", "SOS_PUT_SIGNAL(shmem_putmem_signal_nbi, void, 1, 1)",
                 "SOS_WAIT_UNTIL_SOME_VECTOR(shmem_short_wait_until_some_vector, short, 1)",
                 "SOS_TEST(shmem_ushort_test, unsigned short, 0)", "SOS_WAIT(shmem_longlong_wait, long long)",
                 "SOS_TEST_ANY(shmem_ptrdiff_test_any, ptrdiff_t, 1)", "SOS_WAIT_UNTIL(shmem_size_wait_until, size_t, 0)"):
        assert want in lines, want
    assert ('SOS_ENTRY(void, shmemx_signal_add, (uint64_t *sig_addr, uint64_t signal, int pe), '
            'sos_api_signal_op(sig_addr, signal, SOSX_SIGNAL_ADD, pe, "shmemx_signal_add");)') in lines
    macros = "\n".join(g.signal_macros())
    assert ("return sos_api_wait(vars, nelems, indices, status, cmp, values, 1, SOS_SYNC_SOME, sizeof(T), sg, NULL, "
            "#name);") in macros
    assert "return (int)sos_api_test(var, 1, NULL, NULL, cmp, &value, 0, SOS_SYNC_ONE, sizeof(T), sg, #name);" in macros
    assert "sos_api_put_signal(target, source, nelems, size, sig_addr, signal, sig_op, pe, nbi, #name);" in macros
    # every name has exactly one line of its own
    for n in golden_names():
        assert sum(1 for ln in lines if re.search(rf"[(, ]p?{n}[,(]", ln)) >= 1, n


def test_constants_have_the_references_values():
    text = open(os.path.join(INC, "shmem_signal.h")).read() + open(os.path.join(INC, "shmem_sync.h")).read()
    for name, value in (("SHMEM_SIGNAL_SET", 0), ("SHMEM_SIGNAL_ADD", 1), ("SHMEM_CMP_EQ", 1), ("SHMEM_CMP_NE", 2),
                        ("SHMEM_CMP_GT", 3), ("SHMEM_CMP_GE", 4), ("SHMEM_CMP_LT", 5), ("SHMEM_CMP_LE", 6)):
        assert re.search(rf"^#define {name} {value}$", text, re.M), name
    sosx = open(os.path.join(INC, "sosx.h")).read()
    assert re.search(r"^#define SOSX_SIGNAL_SET 0 ", sosx, re.M) and re.search(r"^#define SOSX_SIGNAL_ADD 1 ", sosx, re.M)


CONSTANTS = '''_Static_assert(SHMEM_SIGNAL_SET == 0 && SHMEM_SIGNAL_ADD == 1, "signal ops");
_Static_assert(SHMEM_CMP_EQ == 1 && SHMEM_CMP_NE == 2 && SHMEM_CMP_GT == 3 && SHMEM_CMP_GE == 4 && SHMEM_CMP_LT == 5 &&
               SHMEM_CMP_LE == 6 && _SHMEM_CMP_LE == 6, "comparisons");
'''
# every arm of the put_signal generics (14 base RMA types), both forms
PUT_USES = "static uint64_t sg;\n" + "".join(
    f"static {ct} d{i}[2], s{i}[2]; shmem_put_signal(d{i}, s{i}, 2, &sg, 1, SHMEM_SIGNAL_SET, 0); "
    f"shmem_put_signal_nbi(d{i}, (const {ct} *)s{i}, 2, &sg, 1, SHMEM_SIGNAL_ADD, 0);\n"
    for i, ct in enumerate(["float", "double", "long double", "char", "signed char", "short", "int", "long", "long long",
                            "unsigned char", "unsigned short", "unsigned int", "unsigned long", "unsigned long long"]))
PUT_USES += '''shmem_put64_signal(d1, s1, 2, &sg, 1, SHMEM_SIGNAL_SET, 0); shmem_putmem_signal_nbi(d1, s1, 16, &sg, 1, SHMEM_SIGNAL_ADD, 0);
pshmem_size_put_signal((size_t *)d12, (const size_t *)s12, 2, &sg, 1, SHMEM_SIGNAL_SET, 0);
sg = shmem_signal_fetch(&sg); shmemx_signal_add(&sg, 1, 0); shmemx_signal_set(&sg, 1, 0);
sg = shmem_signal_wait_until(&sg, SHMEM_CMP_GE, 0);
'''


def sync_uses(types):
    out = ["static int st[2]; static size_t ix[2], n;"]
    for i, ct in enumerate(types):
        v = f"v{i}"
        out.append(f"static {ct} {v}[2]; static int r{i};")
        out.append(f"shmem_wait_until({v}, SHMEM_CMP_EQ, 0); shmem_wait_until_all({v}, 2, st, SHMEM_CMP_EQ, 0); "
                   f"n = shmem_wait_until_any({v}, 2, st, SHMEM_CMP_EQ, 0); n = shmem_wait_until_some({v}, 2, ix, st, SHMEM_CMP_EQ, 0); "
                   f"shmem_wait_until_all_vector({v}, 2, st, SHMEM_CMP_EQ, {v}); n = shmem_wait_until_any_vector({v}, 2, st, SHMEM_CMP_EQ, {v}); "
                   f"n = shmem_wait_until_some_vector({v}, 2, ix, st, SHMEM_CMP_EQ, {v});")
        out.append(f"r{i} = shmem_test({v}, SHMEM_CMP_EQ, 0); r{i} = shmem_test_all({v}, 2, st, SHMEM_CMP_EQ, 0); "
                   f"n = shmem_test_any({v}, 2, st, SHMEM_CMP_EQ, 0); n = shmem_test_some({v}, 2, ix, st, SHMEM_CMP_EQ, 0); "
                   f"r{i} = shmem_test_all_vector({v}, 2, st, SHMEM_CMP_EQ, {v}); n = shmem_test_any_vector({v}, 2, st, SHMEM_CMP_EQ, {v}); "
                   f"n = shmem_test_some_vector({v}, 2, ix, st, SHMEM_CMP_EQ, {v}); (void)r{i};")
    out.append("static uint32_t u32[2]; static ptrdiff_t pd[2]; shmem_uint32_wait_until(u32, SHMEM_CMP_NE, 1); "
               "n = pshmem_ptrdiff_test_some_vector(pd, 2, ix, st, SHMEM_CMP_LT, pd); (void)n;")
    return "\n".join(out) + "\n"


BASE6 = ["int", "long", "long long", "unsigned int", "unsigned long", "unsigned long long"]
SHORTS = ["short", "unsigned short"]   # arms of the C11 selectors only, as in the reference's tables


def _build(tmp_path, lang, body, flags=(), prelude=""):
    ext = "c" if lang == "c" else "cpp"
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\n#include <shmemx.h>\n" + prelude + "int main(void){ shmem_init();\n" + body +
                   "shmem_finalize(); return 0; }\n")
    cc = "gcc" if lang == "c" else "g++"
    std = ["-std=c11"] if lang == "c" else ["-std=c++17"]
    cmd = [cc, *std, "-Wall", "-Werror", *flags, "-I", INC, str(src), "-o", str(tmp_path / "a.out"), "-L",
           os.path.dirname(LIB), "-lsos_amd", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-L/opt/rocm/lib", "-lamdhip64"]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.parametrize("lang", ["c", "cxx"])
def test_generics_compile_and_link(tmp_path, lang):
    body = PUT_USES + sync_uses(BASE6 + (SHORTS if lang == "c" else []))
    r = _build(tmp_path, lang, body, prelude=CONSTANTS if lang == "c" else CONSTANTS.replace("_Static_assert", "static_assert"))
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_has_no_short_overload_as_the_reference():
    g = gen()
    assert [st for st, _ in g.SYNC_GENERIC_C11] == ["short", "int", "long", "longlong", "ushort", "uint", "ulong", "ulonglong"]
    assert [st for st, _ in g.SYNC_GENERIC_CXX] == ["int", "long", "longlong", "uint", "ulong", "ulonglong"]


@pytest.mark.parametrize("lang", ["c", "cxx"])
def test_deprecated_waits_compile_and_warn(tmp_path, lang):
    body = ("static short s; static int i; static long l; static long long ll;\n"
            "shmem_short_wait(&s, 1); shmem_int_wait(&i, 1); shmem_long_wait(&l, 1); shmem_longlong_wait(&ll, 1); shmem_wait(&l, 1);\n")
    r = _build(tmp_path, lang, body, flags=["-Wno-deprecated-declarations"])
    assert r.returncode == 0, r.stderr[-3000:]
    r = _build(tmp_path, lang, "static long l; shmem_long_wait(&l, 1);\n")
    assert r.returncode != 0 and "deprecated" in r.stderr, r.stderr[-2000:]
    r = _build(tmp_path, lang, "static long l; shmem_wait(&l, 1);\n")
    assert r.returncode != 0 and "deprecated" in r.stderr, r.stderr[-2000:]


def test_untyped_wait_until_only_without_the_generics(tmp_path):
    """C99 sees the function shmem_wait_until(long *, int, long); C11 sees the selector, which
    has no arm for a float."""
    src = tmp_path / "t.c"
    src.write_text("#include <shmem.h>\nint main(void){ static long l; shmem_wait_until(&l, SHMEM_CMP_EQ, 0); "
                   "void (*f)(long *, int, long) = shmem_wait_until; (void)f; return 0; }\n")
    cmd = ["gcc", "-Wall", "-Werror", "-I", INC, "-c", str(src), "-o", str(tmp_path / "t.o")]
    assert subprocess.run(cmd + ["-std=c99"], capture_output=True, text=True).returncode == 0
    r = subprocess.run(cmd + ["-std=c11"], capture_output=True, text=True)
    assert r.returncode != 0   # the name is a function-like macro there, not a function


def test_python_mirrors():
    from sos_amd import shmem as S
    c = ctypes
    f = S.shmem_double_put_signal_nbi
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint64, c.c_int, c.c_int]
    assert S.shmem_put32_signal.argtypes == f.argtypes and S.shmem_putmem_signal.argtypes == f.argtypes
    f = S.shmem_short_wait_until
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_int, c.c_short]
    f = S.shmem_uint64_test
    assert f.restype is c.c_int and f.argtypes == [c.c_void_p, c.c_int, c.c_uint64]
    f = S.shmem_long_wait_until_all
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_size_t, c.c_void_p, c.c_int, c.c_long]
    f = S.shmem_int_test_all_vector
    assert f.restype is c.c_int and f.argtypes == [c.c_void_p, c.c_size_t, c.c_void_p, c.c_int, c.c_void_p]
    f = S.shmem_size_wait_until_any
    assert f.restype is c.c_size_t and f.argtypes == [c.c_void_p, c.c_size_t, c.c_void_p, c.c_int, c.c_size_t]
    f = S.shmem_ptrdiff_test_some_vector
    assert f.restype is c.c_size_t and f.argtypes == [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]
    f = S.shmem_longlong_wait
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_longlong]
    assert S.shmem_signal_fetch.restype is c.c_uint64 and S.shmem_signal_wait_until.restype is c.c_uint64
    assert len(S.sos_api_put_signal.argtypes) == 10 and len(S.sos_api_wait.argtypes) == 12
    assert len(S.sos_api_test.argtypes) == 11 and len(S.sos_sync_eval.argtypes) == 12
    assert len(S.sosx_put_signal.argtypes) == 7 and len(S.sosx_sync_snapshot.argtypes) == 5
    for n in golden_names():
        assert getattr(S, n).argtypes is not None, n
    # the older families' mirrors are still their own
    assert len(S.shmem_float_put.argtypes) == 4 and S.shmem_long_g.restype is c.c_long
    assert S.shmem_long_atomic_fetch_add.argtypes == [c.c_void_p, c.c_long, c.c_int]
    with pytest.raises(AttributeError):
        S.shmem_float_wait_until
