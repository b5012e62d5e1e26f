"""CPU: the communication-context surface: every name exported by libsos_amd_ctx.so with its
pshmem_ twin (strong) and shmem_ form (weak) over the sos_api_ctx_* entries of libsos_amd.so,
the committed name list with its per-family counts, the generated headers -- which stamp each
form over type tables -- declaring exactly those prototypes once preprocessed, the generics
taking a leading shmem_ctx_t compiled as C11 and C++ with each used once, the Python mirrors,
and -- where the reference tree is present -- the prototypes against its m4 declarations."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")
CTXLIB = os.path.join(ROOT, "sos_amd", "libsos_amd_ctx.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctx_symbols.txt")
REF = "/root/reference"
MANAGEMENT = ["shmem_ctx_create", "shmem_ctx_destroy", "shmem_ctx_quiet", "shmem_ctx_fence", "shmem_team_create_ctx",
              "shmem_ctx_get_team"]
DEPRECATED = ("cswap", "finc", "inc", "fadd", "add", "swap", "fetch", "set")


def symbol_kinds(lib=LIB):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True,
                         check=True).stdout
    return {ln.split()[2]: ln.split()[1] for ln in out.splitlines() if len(ln.split()) == 3}


def gen():
    sys.path.insert(0, os.path.join(ROOT, "sos_amd", "csrc"))
    import gen_bindings
    return gen_bindings


def golden_names():
    return open(GOLDEN).read().split()


def plain(name):
    return name.replace("_ctx_", "_", 1)


def test_name_list_is_the_generators():
    g = gen()
    names = golden_names()
    assert sorted(g.ctx_symbols()) == names and len(set(names)) == len(names)
    twins = [n for n in names if n not in MANAGEMENT]
    assert sorted(set(names) - set(twins)) == sorted(MANAGEMENT)
    assert all(re.match(r"shmemx?_ctx_", n) for n in twins)
    # every one-sided name but shmem_ptr, every non-deprecated atomic, put with signal and the
    # two signal operations -- counted from the plain families' own lists
    rma = {n for n in g.rma_symbols() if n != "shmem_ptr"}
    amo = {n for n, _, _, dep in g.amo_entries() if not dep}
    sig = {n for n in g.signal_symbols() if re.search(r"put(\d+|mem)?_signal(_nbi)?$", n)} | {"shmemx_signal_add",
                                                                                             "shmemx_signal_set"}
    assert (len(rma), len(sig)) == (284, 62)
    assert len(amo) == len(g.amo_symbols()) - sum(
        len(g.AMO_TABLES[g.AMO_FORMS[f][0]]) for f in DEPRECATED)
    assert {plain(n) for n in twins} == rma | amo | sig and len(twins) == len(rma) + len(amo) + len(sig)
    for n in ("shmem_ctx_float_put", "shmem_ctx_get128_nbi", "shmem_ctx_putmem", "shmem_ctx_longdouble_g",
              "shmemx_ctx_ptrdiff_ibput", "shmemx_ctx_ibget64", "shmem_ctx_double_atomic_fetch_nbi",
              "shmem_ctx_uint32_atomic_fetch_xor_nbi", "shmem_ctx_size_put_signal_nbi", "shmem_ctx_putmem_signal",
              "shmemx_ctx_signal_add", "shmemx_ctx_signal_set"):
        assert n in names, n
    # what SOS has no ctx form of
    for n in ("shmem_ctx_ptr", "shmem_ctx_long_fadd", "shmem_ctx_int_cswap", "shmem_ctx_signal_fetch",
              "shmem_ctx_long_wait_until", "shmem_ctx_int_test", "shmem_ctx_signal_wait_until", "shmem_ctx_set_lock",
              "shmem_ctx_float_atomic_add"):
        assert n not in names, n


def test_ctx_symbols_exported_strong_and_weak():
    kinds, ckinds = symbol_kinds(), symbol_kinds(CTXLIB)
    wrong = [n for n in golden_names() if ckinds.get("p" + n) != "T" or ckinds.get(n) != "W"]
    assert not wrong, wrong[:10]
    # the list is all the companion library exports
    exported = {n for n in ckinds if "shmem" in n}
    assert exported == set(golden_names()) | {"p" + n for n in golden_names()}, sorted(exported)[:5]
    # the runtime holds the entries behind them, no public ctx name, and not the test hook
    for n in ("sos_api_ctx_create", "sos_api_ctx_destroy", "sos_api_ctx_quiet", "sos_api_ctx_fence",
              "sos_api_team_create_ctx", "sos_api_ctx_get_team", "sos_api_ctx_put", "sos_api_ctx_get", "sos_api_ctx_iput",
              "sos_api_ctx_iget", "sos_api_ctx_ibput", "sos_api_ctx_ibget", "sos_api_ctx_p", "sos_api_ctx_g",
              "sos_api_ctx_amo", "sos_api_ctx_put_signal", "sos_api_ctx_signal_op", "sos_ctx_check",
              "sos_ctx_options_check", "sos_ctx_pool_size", "sos_ctx_stream_slot", "sosx_put_signal_on",
              "sosx_ctx_streams"):
        assert kinds.get(n) == "T", n
    assert kinds.get("SHMEM_CTX_DEFAULT") in ("B", "D"), kinds.get("SHMEM_CTX_DEFAULT")
    assert not [n for n in kinds if "shmem_ctx_" in n or "shmemx_ctx_" in n]
    assert "sosx_ctx_stats" not in kinds
    # every sos_api_ the companion needs is the runtime's
    und = subprocess.run(["nm", "-D", "--undefined-only", CTXLIB], capture_output=True, text=True, check=True).stdout
    need = {ln.split()[-1] for ln in und.splitlines() if "sos_api_" in ln}
    assert need and all(kinds.get(n) == "T" for n in need), sorted(n for n in need if kinds.get(n) != "T")


def preprocessed(lang):
    """shmem.h and shmemx.h as the compiler sees them."""
    cmd = ["gcc", "-E", "-P", "-x", "c" if lang == "c" else "c++", "-std=c11" if lang == "c" else "-std=c++17",
           "-I", INC, "-"]
    r = subprocess.run(cmd, input="#include <shmem.h>\n#include <shmemx.h>\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("lang", ["c", "cxx"])
def test_headers_declare_exactly_the_names(lang):
    """The headers stamp each form over type tables: once preprocessed they declare every
    generated prototype, shmem_ and pshmem_, and no other context name."""
    g = gen()
    raw = preprocessed(lang)
    text = re.sub(r"\s+", "", raw)
    protos = [sig for _, _, _, sig in g.ctx_entries()]
    protos += [lambda p, n=n, r=r, a=a: f"{r} {p}{n}({a})" for n, r, a, _ in g.CTX_MANAGEMENT]
    missing = [sig("") for sig in protos for p in ("", "p") if re.sub(r"\s+", "", sig(p)) + ";" not in text]
    assert not missing, missing[:5]
    # a declaration names its first parameter's type; a call in an overload's body does not
    declared = set(re.findall(r"\b(p?shmemx?_(?:team_create_ctx|ctx_\w+))\s*\(\s*(?:shmem_ctx_t|shmem_team_t|long)\s", raw))
    want = set(golden_names()) | {"p" + n for n in golden_names()}
    assert declared == want, sorted(declared ^ want)[:10]
    # included last, after every header whose generics they redefine
    shmem_h = open(os.path.join(INC, "shmem.h")).read()
    shmemx_h = open(os.path.join(INC, "shmemx.h")).read()
    assert shmem_h.rindex('#include "') == shmem_h.index('#include "shmem_ctx.h"')
    assert shmemx_h.rindex('#include "') == shmemx_h.index('#include "shmemx_ctx.h"')
    # SOS's values (mpp/shmem-def.h.in)
    for name, value in (("SHMEM_CTX_PRIVATE", "(1l << 0)"), ("SHMEM_CTX_SERIALIZED", "(1l << 1)"),
                        ("SHMEM_CTX_NOSTORE", "(1l << 2)"), ("SHMEM_CTX_INVALID", "NULL")):
        assert re.search(rf"^#define {name}\s+{re.escape(value)}$", shmem_h, re.M), name
    assert "extern shmem_ctx_t SHMEM_CTX_DEFAULT;" in shmem_h


def test_generated_ctx_bindings_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sos_amd", "csrc", "gen_bindings.py"), "--check"])
    assert r.returncode == 0
    g = gen()
    src = open(os.path.join(ROOT, "sos_amd", "csrc", "ctx_gen.cpp")).read()
    assert src == g.ctx_source()
    assert open(os.path.join(INC, "shmem_ctx.h")).read() == g.ctx_header("shmem")
    assert open(os.path.join(INC, "shmemx_ctx.h")).read() == g.ctx_header("shmemx")
    # one line per form, each over its entry behind the context
    assert ("SOS_CTX_DEF(void, shmem_ctx_##N##_put_nbi, (shmem_ctx_t ctx, T *target, const T *source, size_t nelems, "
            "int pe), sos_api_ctx_put(ctx, target, source, nelems, sizeof(T), pe, 1, fn);)") in src
    assert ("SOS_CTX_DEF(T, shmem_ctx_##N##_atomic_fetch_add, (shmem_ctx_t ctx, T *target, T value, int pe), T old; "
            "sos_api_ctx_amo(ctx, SOSX_AMO_ADD, target, &value, NULL, &old, 1, sizeof(T), (T)0.5 != (T)0, pe, 0, fn); "
            "return old;)") in src
    assert ("SOS_CTX_DEF(void, shmem_ctx_put##N##_signal_nbi, (shmem_ctx_t ctx, void *target, const void *source, "
            "size_t nelems, uint64_t *sig_addr, uint64_t signal, int sig_op, int pe), sos_api_ctx_put_signal(ctx, target, "
            "source, nelems, SZ, sig_addr, signal, sig_op, pe, 1, fn);)") in src
    assert ("SOS_CTX_DEF(void, shmemx_ctx_signal_set, (shmem_ctx_t ctx, uint64_t *sig_addr, uint64_t signal, int pe), "
            "sos_api_ctx_signal_op(ctx, sig_addr, signal, SOSX_SIGNAL_SET, pe, fn);)") in src
    # the stamped tables are the generator's
    hdr = open(os.path.join(INC, "shmem_ctx.h")).read()
    for table, rows in g.CTX_TABLES.items():
        assert f"#define SHMEM_CTX_FOR_{table}(X) " + " ".join(f"X({a}, {b})" for a, b in rows) + "\n" in hdr, table


# every generic with a leading context once, next to its plain use
USES = '''static long a[16], b[16]; static double d[16], e[16]; static char c[16], f[16];
static long double x[4], y[4]; static unsigned short us[8], ut[8]; static uint64_t sig;
shmem_ctx_t ctx = SHMEM_CTX_INVALID; shmem_team_t team = SHMEM_TEAM_INVALID;
if (shmem_ctx_create(SHMEM_CTX_PRIVATE | SHMEM_CTX_SERIALIZED | SHMEM_CTX_NOSTORE, &ctx)) return 1;
if (shmem_ctx_get_team(ctx, &team)) return 1;
shmem_put(ctx, a, b, 1, 0); shmem_get(ctx, d, e, 2, 0); shmem_put_nbi(ctx, c, f, 3, 0); shmem_get_nbi(ctx, x, y, 1, 0);
shmem_p(ctx, a, 5L, 0); long v = shmem_g(ctx, a, 0); const double *ce = e; double w = shmem_g(ctx, ce, 0);
shmem_iput(ctx, us, ut, 2, 1, 3, 0); shmem_iget(ctx, d, e, 1, 2, 3, 0);
shmemx_ibput(ctx, a, b, 4, 4, 2, 2, 0); shmemx_ibget(ctx, d, e, 4, 4, 2, 2, 0);
shmem_put(a, b, 1, 0); shmem_p(a, 5L, 0); v += shmem_g(a, 0); w += shmem_g(ce, 0); shmemx_ibput(a, b, 4, 4, 2, 2, 0);
shmem_ctx_put64(ctx, a, b, 1, 0); shmem_ctx_get8(ctx, c, f, 1, 0); shmem_ctx_iput128(ctx, x, y, 1, 1, 1, 0);
shmem_ctx_putmem_nbi(ctx, a, b, 8, 0); shmemx_ctx_ibget32(ctx, a, b, 4, 4, 2, 2, 0);
pshmem_ctx_long_put(ctx, a, b, 1, 0); pshmemx_ctx_long_ibget(ctx, a, b, 4, 4, 2, 2, 0);
static int i; static long l; static long long ll; static unsigned u; static unsigned long ul;
static unsigned long long ull; static float fl; static double db; static const double cd = 1.0;
static int fi; static long fL; static float ff; static double fd; static unsigned fu; static unsigned long ful;
i = shmem_atomic_compare_swap(ctx, &i, 0, 1, 0); l = shmem_atomic_fetch_inc(ctx, &l, 0); shmem_atomic_inc(ctx, &ll, 0);
u = shmem_atomic_fetch_add(ctx, &u, 2u, 0); shmem_atomic_add(ctx, &ul, 3ul, 0);
shmem_atomic_compare_swap_nbi(ctx, &fi, &i, 0, 1, 0); shmem_atomic_fetch_inc_nbi(ctx, &fL, &l, 0);
shmem_atomic_fetch_add_nbi(ctx, &fu, &u, 2u, 0);
fl = shmem_atomic_swap(ctx, &fl, 1.5f, 0); db = shmem_atomic_fetch(ctx, &db, 0); db = shmem_atomic_fetch(ctx, &cd, 0);
shmem_atomic_set(ctx, &ull, 4ull, 0); shmem_atomic_swap_nbi(ctx, &ff, &fl, 2.5f, 0);
shmem_atomic_fetch_nbi(ctx, &fd, &db, 0); shmem_atomic_fetch_nbi(ctx, &fd, &cd, 0);
shmem_atomic_and(ctx, &u, 1u, 0); shmem_atomic_or(ctx, &ul, 1ul, 0); shmem_atomic_xor(ctx, &ull, 1ull, 0);
u = shmem_atomic_fetch_and(ctx, &u, 1u, 0); ul = shmem_atomic_fetch_or(ctx, &ul, 1ul, 0);
ull = shmem_atomic_fetch_xor(ctx, &ull, 1ull, 0);
shmem_atomic_fetch_and_nbi(ctx, &fu, &u, 1u, 0); shmem_atomic_fetch_or_nbi(ctx, &ful, &ul, 1ul, 0);
shmem_atomic_fetch_xor_nbi(ctx, &fu, &u, 1u, 0);
i = shmem_atomic_compare_swap(&i, 0, 1, 0); db = shmem_atomic_fetch(&cd, 0); shmem_atomic_fetch_nbi(&fd, &cd, 0);
shmem_atomic_inc(&ll, 0); shmem_atomic_or(&ul, 1ul, 0);
shmem_put_signal(ctx, a, b, 1, &sig, 1, SHMEM_SIGNAL_SET, 0); shmem_put_signal_nbi(ctx, d, e, 1, &sig, 1, SHMEM_SIGNAL_ADD, 0);
shmem_put_signal(a, b, 1, &sig, 1, SHMEM_SIGNAL_SET, 0);
shmem_ctx_putmem_signal(ctx, a, b, 8, &sig, 1, SHMEM_SIGNAL_SET, 0); shmem_ctx_put32_signal_nbi(ctx, a, b, 1, &sig, 1, 0, 0);
shmemx_signal_add(ctx, &sig, 1, 0); shmemx_signal_set(ctx, &sig, 1, 0); shmemx_signal_add(&sig, 1, 0);
shmemx_ctx_signal_set(ctx, &sig, 2, 0); pshmemx_ctx_signal_add(ctx, &sig, 2, 0);
shmem_ctx_fence(ctx); shmem_ctx_quiet(ctx); shmem_ctx_quiet(SHMEM_CTX_DEFAULT); shmem_ctx_destroy(ctx);
if (shmem_team_create_ctx(SHMEM_TEAM_WORLD, 0, &ctx) == 0) pshmem_ctx_destroy(ctx);
(void)v; (void)w;
'''
USES_C11_ONLY = '''static int32_t i32; static int64_t j64; static int32_t fi32;
shmem_atomic_and(SHMEM_CTX_DEFAULT, &i32, 1, 0); j64 = shmem_atomic_fetch_or(SHMEM_CTX_DEFAULT, &j64, 1, 0);
shmem_atomic_fetch_xor_nbi(SHMEM_CTX_DEFAULT, &fi32, &i32, 1, 0);
'''


@pytest.mark.parametrize("lang,ext", [("c", "c"), ("cxx", "cpp")])
def test_ctx_generics_compile_and_link(tmp_path, lang, ext):
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\n#include <shmemx.h>\nint main(void){ shmem_init();\n" + USES +
                   (USES_C11_ONLY if lang == "c" else "") + "shmem_finalize(); return 0; }\n")
    cc = "gcc" if lang == "c" else "g++"
    std = ["-std=c11"] if lang == "c" else ["-std=c++17"]
    cmd = [cc, *std, "-Wall", "-Werror", "-I", INC, str(src), "-o", str(tmp_path / "a.out"), "-L",
           os.path.dirname(LIB), "-lsos_amd_ctx", "-lsos_amd", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_a_wrong_type_behind_a_context_does_not_compile(tmp_path):
    """The inner selector has no arm for it: SOS's selection-failed function takes no arguments."""
    src = tmp_path / "t.c"
    src.write_text("#include <shmem.h>\nint main(void){ static _Bool a[2], b[2]; "
                   "shmem_put(SHMEM_CTX_DEFAULT, a, b, 1, 0); return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, "-c", str(src), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "shmem_ctx_c11_generic_selection_failed" in r.stderr, r.stderr[-2000:]


def test_python_mirrors():
    from sos_amd import shmem as S
    c = ctypes
    assert S.shmem_ctx_create.restype is c.c_int and len(S.shmem_ctx_create.argtypes) == 2
    assert S.shmem_team_create_ctx.restype is c.c_int and len(S.shmem_team_create_ctx.argtypes) == 3
    assert S.shmem_ctx_get_team.restype is c.c_int and S.shmem_ctx_destroy.restype is None
    assert S.shmem_ctx_quiet.argtypes == [c.c_void_p] and S.shmem_ctx_fence.argtypes == [c.c_void_p]
    f = S.shmem_ctx_float_put
    assert f.restype is None and f.argtypes == [c.c_void_p] + S.shmem_float_put.argtypes and len(f.argtypes) == 5
    f = S.shmem_ctx_long_atomic_fetch_add
    assert f.restype is c.c_long and f.argtypes == [c.c_void_p, c.c_void_p, c.c_long, c.c_int]
    f = S.shmem_ctx_double_atomic_fetch_nbi
    assert f.restype is None and f.argtypes == [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int]
    assert S.shmem_ctx_longdouble_g.restype is c.c_longdouble and len(S.shmemx_ctx_ibget64.argtypes) == 8
    assert len(S.shmem_ctx_int_put_signal_nbi.argtypes) == 8 and len(S.shmemx_ctx_signal_add.argtypes) == 4
    # every name resolves with a leading handle and its plain form's arguments behind it
    for n in golden_names():
        if n in MANAGEMENT:
            continue
        f, g = getattr(S, n), getattr(S, plain(n))
        assert f.restype is g.restype and f.argtypes == [c.c_void_p] + list(g.argtypes), n
    for n in ("shmem_ctx_long_fadd", "shmem_ctx_set_lock", "shmem_ctx_long_wait_until", "shmem_ctx_signal_fetch"):
        with pytest.raises(AttributeError):
            getattr(S, n)
    # the entries the existing tests pin keep their argument counts
    for n, k in (("sos_api_put", 7), ("sos_api_iput", 8), ("sos_api_ibput", 9), ("sos_api_p", 5), ("sos_api_amo", 11),
                 ("sos_api_put_signal", 10), ("sos_api_signal_op", 5), ("sosx_put_signal", 7)):
        assert len(getattr(S, n).argtypes) == k, n
    assert S.sosx_ctx_streams() == 3 and (S.SHMEM_CTX_PRIVATE, S.SHMEM_CTX_SERIALIZED, S.SHMEM_CTX_NOSTORE) == (1, 2, 4)


def _m4_args(text):
    """Parameter types of an m4 prototype body: names dropped, $2 kept."""
    args = [re.sub(r"\s+", " ", a.strip()) for a in text.split(",")]
    return [re.sub(r"\s*\b\w+$", "", a).replace(" *", "*").replace("* ", "*").strip() for a in args]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present")
def test_prototypes_match_the_reference_tables():
    """Every generated ctx prototype, and the six management calls, against the reference's m4
    declaration of the same form: return type and parameter types.  The counts come from the
    reference's own tables: every ctx declaration it makes over a type table is matched by
    exactly the names that table gives."""
    g = gen()
    decls = {}
    for path in ("mpp/shmem_c_func.h4", "mpp/shmemx_c_func.h4"):
        text = re.sub(r"SH_PAD\(`\$1'\)", "", open(os.path.join(REF, path)).read())
        for m in re.finditer(r"SHMEM_FUNCTION_ATTRIBUTES\s+([\w$ ]+?\*?)\s*SHPRE\(\)(shmemx?_[\w$]+)\(([^)]*)\)([^'\n]*)", text):
            ret, name, args, tail = m.groups()
            decls[name] = (ret.strip(), _m4_args(args), "SHMEM_ATTRIBUTE_DEPRECATED" in tail)
    for name, ret, params, _ in g.CTX_MANAGEMENT:
        assert decls[name][:2] == (ret, _m4_args(params)), name
    types = dict(g.RMA) | dict(g.EXTENDED_AMO)
    used, per_family = set(), {"rma": 0, "amo": 0, "signal": 0}
    for hdr, family, name, sig in g.ctx_entries():
        ret, rest = sig("").split(name + "(")
        mine = _m4_args(rest.rstrip(")"))
        cands = []
        m = re.fullmatch(r"(shmemx?_ctx)_([a-z0-9]+?)_(\w+)", name)
        if m and m.group(2) in types:
            cands.append((f"{m.group(1)}_$1_{m.group(3)}", types[m.group(2)]))
        m2 = re.fullmatch(r"(shmemx?_ctx_[a-z]+?)(\d+|mem)((?:_signal)?(?:_nbi)?)", name)
        if m2:
            cands.append((f"{m2.group(1)}$1{m2.group(3)}", None))
        cands.append((name, None))
        for key, ct in cands:
            if key in decls:
                rret, rargs, rdep = decls[key]
                if ct:
                    rret, rargs = rret.replace("$2", ct), [a.replace("$2", ct) for a in rargs]
                assert ret.strip() == rret and mine == rargs and not rdep, (name, ret, rret, mine, rargs)
                used.add(key)
                per_family[family] += 1
                break
        else:
            raise AssertionError(f"{name}: no declaration in the reference")
    # nothing the reference declares for a context is missing here, but for what is out of scope
    ref_ctx = {k for k in decls if "_ctx_" in k} - set(MANAGEMENT)
    assert ref_ctx == used, sorted(ref_ctx ^ used)
    # the atomics' count from the reference's tables, not from a number written down
    bind = open(os.path.join(REF, "bindings/shmem_bind_c.m4")).read()

    def table_len(macro):
        return len(re.findall(r"\$1\(", bind.split(f"define(`{macro}'")[1].split("')dnl")[0]))

    n_amo, n_ext, n_bit = table_len("SHMEM_BIND_C_AMO"), table_len("SHMEM_BIND_C_EXTENDED_AMO"), \
        table_len("SHMEM_BIND_C_BITWISE_AMO")
    text = open(os.path.join(REF, "mpp/shmem_c_func.h4")).read()
    want_amo = 0
    for macro, n in (("SHMEM_DECLARE_FOR_AMO", n_amo), ("SHMEM_DECLARE_FOR_EXTENDED_AMO", n_amo + n_ext),
                     ("SHMEM_DECLARE_FOR_BITWISE_AMO", n_bit)):
        for form in re.findall(macro + r"\(`(SHMEM_C_\w+)'\)", text):
            body = text.split(f"define(`{form}'")[1].split("')dnl")[0]
            want_amo += n * len(re.findall(r"SHPRE\(\)shmem_ctx_\$1_", body))
    assert per_family["amo"] == want_amo > 0, (per_family, want_amo)
    assert per_family["rma"] == len(g.rma_symbols()) - 1 and per_family["signal"] == 62, per_family
