"""CPU: the distributed locks' surface: the three names exported with their pshmem_ twins
(strong) and shmem_ forms (weak), the committed name list, include/shmem_lock.h compiled as
C11 and C++ with each function used once, the prototypes equal to the reference's text
(mpp/shmem_c_func.h4), no context form anywhere, and the Python mirrors."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "sos_amd", "libsos_amd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lock_symbols.txt")
REF_H4 = "/root/reference/mpp/shmem_c_func.h4"
NAMES = ["shmem_clear_lock", "shmem_set_lock", "shmem_test_lock"]


def symbol_kinds():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2]: ln.split()[1] for ln in out.splitlines() if len(ln.split()) == 3}


def golden_names():
    return open(GOLDEN).read().split()


def header_prototypes():
    """name -> (return type, parameter list), whitespace normalised, of every function shmem_lock.h declares"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "shmem_lock.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^(?:SHMEM_FUNCTION_ATTRIBUTES\s+)?([\w ]+?)\s*\b(p?shmem_\w+)\(([^)]*)\);", text, re.M):
        out[m.group(2)] = (m.group(1).strip(), re.sub(r"\s+", " ", m.group(3).strip()))
    return out


def test_name_list():
    assert golden_names() == NAMES
    protos = header_prototypes()
    assert sorted(protos) == sorted(NAMES + ["p" + n for n in NAMES])
    for n in NAMES:
        assert protos[n] == protos["p" + n], n
    shmem_h = open(os.path.join(INC, "shmem.h")).read()
    assert shmem_h.index('#include "shmem_sync.h"') < shmem_h.index('#include "shmem_lock.h"')


def test_symbols_exported_strong_and_weak():
    kinds = symbol_kinds()
    wrong = [n for n in golden_names() if kinds.get("p" + n) != "T" or kinds.get(n) != "W"]
    assert not wrong, wrong
    for n in ("sos_api_set_lock", "sos_api_clear_lock", "sos_api_test_lock", "sos_lock_check",
              "sos_lock_expiry_message", "sos_lock_corrupt_message", "sosx_lock_step", "sosx_lock_table",
              "sosx_lock_stats"):
        assert kinds.get(n) == "T", n
    # three names, six symbols: no typed variant and no context form
    assert sorted(n for n in kinds if re.search(r"(set|clear|test)_lock$", n) and "shmem" in n) == \
        sorted(NAMES + ["p" + n for n in NAMES])
    assert not [n for n in kinds if "shmem_ctx_" in n]


@pytest.mark.skipif(not os.path.exists(REF_H4), reason="reference checkout not present")
def test_prototypes_are_the_references():
    text = open(REF_H4).read()
    protos = header_prototypes()
    for n in NAMES:
        m = re.search(r"^SHMEM_FUNCTION_ATTRIBUTES\s+([\w ]+?)\s*SHPRE\(\)" + n + r"\(([^)]*)\);", text, re.M)
        assert m, n
        assert protos[n] == (m.group(1).strip(), re.sub(r"\s+", " ", m.group(2).strip())), n
    assert "shmem_ctx_set_lock" not in text and "shmem_ctx_test_lock" not in text   # the reference has none either


USES = ("static long lock;\nshmem_set_lock(&lock); shmem_clear_lock(&lock);\n"
        "if (shmem_test_lock(&lock) == 0) pshmem_clear_lock(&lock);\n"
        "pshmem_set_lock(&lock); if (pshmem_test_lock(&lock)) shmem_clear_lock(&lock);\n"
        "void (*f)(long *) = shmem_set_lock; int (*g)(long *) = shmem_test_lock; (void)f; (void)g;\n")


@pytest.mark.parametrize("lang", ["c", "cxx"])
def test_header_compiles_and_links(tmp_path, lang):
    ext = "c" if lang == "c" else "cpp"
    src = tmp_path / f"t.{ext}"
    src.write_text("#include <shmem.h>\nint main(void){ shmem_init();\n" + USES + "shmem_finalize(); return 0; }\n")
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    cmd = [cc, std, "-Wall", "-Werror", "-pedantic", "-I", INC, str(src), "-o", str(tmp_path / "a.out"), "-L",
           os.path.dirname(LIB), "-lsos_amd", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_sosx_constants():
    sosx = open(os.path.join(INC, "sosx.h")).read()
    for name, value in (("SOSX_LOCK_ENQUEUE", 0), ("SOSX_LOCK_TRY", 1), ("SOSX_LOCK_RELEASE", 2), ("SOSX_LOCK_HANDOFF", 3),
                        ("SOSX_LOCK_ACQUIRED", 0), ("SOSX_LOCK_QUEUED", 1), ("SOSX_LOCK_BUSY", 2), ("SOSX_LOCK_RELEASED", 3),
                        ("SOSX_LOCK_HANDED", 4), ("SOSX_LOCK_PENDING", 5), ("SOSX_LOCK_CORRUPT", 6),
                        ("SOSX_LOCK_RESULT_BYTES", 16)):
        assert re.search(rf"^#define {name}\s+{value}\b", sosx, re.M), name
    # the step functions' own enums carry the same values
    proto = open(os.path.join(ROOT, "sos_amd", "csrc", "lock_proto.h")).read()
    for name, value in (("LOCK_ENQUEUE", 0), ("LOCK_TRY", 1), ("LOCK_RELEASE", 2), ("LOCK_HANDOFF", 3), ("LOCK_ACQUIRED", 0),
                        ("LOCK_QUEUED", 1), ("LOCK_BUSY", 2), ("LOCK_RELEASED", 3), ("LOCK_HANDED", 4), ("LOCK_PENDING", 5),
                        ("LOCK_CORRUPT", 6)):
        assert re.search(rf"\b{name} = {value}\b", proto), name


def test_python_mirrors():
    from sos_amd import shmem as S
    c = ctypes
    assert S.shmem_set_lock.restype is None and S.shmem_set_lock.argtypes == [c.c_void_p]
    assert S.shmem_clear_lock.restype is None and S.shmem_clear_lock.argtypes == [c.c_void_p]
    assert S.shmem_test_lock.restype is c.c_int and S.shmem_test_lock.argtypes == [c.c_void_p]
    assert len(S.sosx_lock_step.argtypes) == 9 and S.sosx_lock_step.restype is c.c_int
    assert len(S.sos_lock_check.argtypes) == 4
    with pytest.raises(AttributeError):
        S.shmem_ctx_set_lock
    with pytest.raises(AttributeError):
        S.shmem_long_set_lock
