"""CPU: the checks of the communication contexts (sos_amd/csrc/onesided_checks.cpp) as plain
functions of data.

(a) tests/ctx_checks_harness.cpp, a program of its own compiled with onesided_checks.cpp -- no HIP,
    no library -- plain and with -fsanitize=address,undefined: the option mask; invalid,
    default, destroyed and unknown handles, looked up and never dereferenced (the handles are
    made-up numbers); the team-index translation for the strided team start 1, stride 2,
    size 3 of 8 PEs (0, 1, 2 -> PEs 1, 3, 5; 3 refused with put / get's bad-PE message); the
    SHMEMX_CTX_STREAMS values; the stream-pool assignment for pools of 1, 3 and 31.
(b) the same functions through the library's exports, and that the file -- which holds every
    check of the one-sided layer -- has no HIP in it.
Nothing is started that could abort."""
import ctypes
import os
import subprocess

import pytest

from sos_amd import shmem as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "build")
CSRC = os.path.join(ROOT, "sos_amd", "csrc")
FLAVOURS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}
OK, BAD_PE, INVALID, DESTROYED, UNKNOWN, BAD_OPTIONS = 0, 2, 14, 15, 16, 17


@pytest.fixture(scope="module", params=list(FLAVOURS))
def harness(request):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, f"ctx_checks_harness_{request.param}")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *FLAVOURS[request.param], "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "ctx_checks_harness.cpp"),
           os.path.join(CSRC, "onesided_checks.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_harness_passes(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=120, env=dict(os.environ, **ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-4000:]
    assert " 0 failed OK" in r.stdout, r.stdout
    assert int(r.stdout.split(":")[1].split()[0]) == 94, r.stdout  # the EXPECTs the harness runs through


def test_file_has_no_hip():
    text = open(os.path.join(CSRC, "onesided_checks.cpp")).read()
    code = text.split('#include "onesided_checks.h"')[1]
    assert "#include <hip" not in text and "hip" not in code and "runtime.h" not in text


class Entry(ctypes.Structure):
    _fields_ = [("handle", ctypes.c_void_p), ("start", ctypes.c_int), ("stride", ctypes.c_int), ("size", ctypes.c_int)]


class Table(ctypes.Structure):
    _fields_ = [("nlive", ctypes.c_int), ("live", ctypes.POINTER(Entry)), ("ndead", ctypes.c_int),
                ("dead", ctypes.POINTER(ctypes.c_void_p))]


def check(handle, pe=None):
    live = (Entry * 3)(Entry(0x1000, 0, 1, 8), Entry(0x2000, 0, 1, 8), Entry(0x3000, 1, 2, 3))
    dead = (ctypes.c_void_p * 1)(0x4000)
    t = Table(3, live, 1, dead)
    msg = ctypes.create_string_buffer(256)
    p, idx = ctypes.c_int(pe if pe is not None else 0), ctypes.c_int(99)
    rc = S.sos_ctx_check(ctypes.addressof(t), handle, ctypes.byref(p) if pe is not None else None, ctypes.byref(idx),
                         msg, 256)
    return rc, p.value, idx.value, msg.value.decode()


def test_exported_checks_agree():
    assert check(None, 0)[0] == INVALID and "SHMEM_CTX_INVALID" in check(None, 0)[3]
    assert check(0x4000, 0)[0] == DESTROYED and check(0x7000, 0)[0] == UNKNOWN
    assert check(0x1000, 5) == (OK, 5, 0, "") and check(0x2000) == (OK, 0, 1, "")
    assert [check(0x3000, i)[:3] for i in range(3)] == [(OK, 1, 2), (OK, 3, 2), (OK, 5, 2)]
    assert check(0x3000, 3) == (BAD_PE, 3, 2, "PE argument (3) is invalid")
    msg = ctypes.create_string_buffer(256)
    assert [S.sos_ctx_options_check(o, msg, 256) for o in (0, 1, 2, 4, 7)] == [OK] * 5
    assert S.sos_ctx_options_check(8, msg, 256) == BAD_OPTIONS and b"options" in msg.value
    assert [S.sos_ctx_pool_size(v, msg, 256) for v in (None, b"1", b"3", b"31", b"0", b"32")] == [3, 1, 3, 31, -1, -1]
    assert [S.sos_ctx_stream_slot(n, 1) for n in range(4)] == [0, 0, 0, 0]
    assert [S.sos_ctx_stream_slot(n, 3) for n in range(5)] == [0, 1, 2, 0, 1]
