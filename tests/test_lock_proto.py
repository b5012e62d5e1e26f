"""CPU: the lock's step functions (sos_amd/csrc/lock_proto.h: enqueue, try_acquire, release,
hand_off) over the CPU atomics backend, in tests/lock_proto_harness.cpp -- a program of its
own, built three ways: plain, with -fsanitize=address,undefined and with -fsanitize=thread.

(a) deterministic scripts against a model of the queue the harness keeps itself: an
    uncontended acquire and release, three PEs queueing 0, 2, 1 and releasing in turn, try on
    a held lock, a release that finds its successor not yet linked (PENDING, nothing changed)
    and the later hand-off, and `last` / NEXT values of 0, n_pes, n_pes + 1, INT_MAX and
    negative: CORRUPT where out of range, and no word outside the P lock words touched (guard
    words; the address sanitizer would report a wild access).
(b) P = 2, 3, 4, 8 threads, each a few thousand rounds of set, counter++ (not atomic), clear,
    some of them through try: the counter is P * rounds and every word zero at the end.  The
    thread sanitizer must stay silent: that checks the memory orders of the step functions.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "build")
FLAVOURS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
            "tsan": ["-O1", "-g", "-fsanitize=thread"]}
ENV = {"TSAN_OPTIONS": "halt_on_error=1 exitcode=66", "ASAN_OPTIONS": "detect_leaks=1",
       "UBSAN_OPTIONS": "halt_on_error=1 print_stacktrace=1"}
ROUNDS = 3000


@pytest.fixture(scope="module", params=list(FLAVOURS))
def harness(request):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, f"lock_proto_harness_{request.param}")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *FLAVOURS[request.param],
           "-I" + os.path.join(ROOT, "sos_amd", "csrc"), os.path.join(ROOT, "tests", "lock_proto_harness.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("ThreadSanitizer", "AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_scripts_match_the_model(harness):
    out = run(harness, "scripts")
    assert "lock_proto scripts:" in out and "checks OK" in out, out
    # uncontended 4 x 14, the 0-2-1 queue 18, try 10, PENDING 13, 7 garbage values x 14
    assert int(out.split(":")[1].split()[0]) >= 56 + 18 + 10 + 13 + 98, out


@pytest.mark.parametrize("P", [2, 3, 4, 8])
def test_threads_count_every_round(harness, P):
    out = run(harness, "threads", P, ROUNDS)
    assert f"P={P} rounds={ROUNDS} counter={P * ROUNDS} " in out and out.rstrip().endswith("OK"), out


def test_header_has_no_hip():
    """The idiom of p2p_proto.h and putsignal_plan.h: the step functions compile without HIP."""
    text = open(os.path.join(ROOT, "sos_amd", "csrc", "lock_proto.h")).read()
    code = text.split("#pragma once")[1]
    assert "#include <hip" not in code and "__hip_" not in code and "__device__" not in code
