"""Multi-PE correctness run of put-with-signal, the signal operations and the point-to-point
waits and tests (one process per PE, tools/oshrun, p2p transport):

  * every generated form once, driven from tests/golden/signal_symbols.txt so none can be
    missed: the put_signal forms against the PE itself and both neighbours (device and
    pageable sources, SET and ADD), the wait / test forms on ivars the neighbours wrote;
  * a ping-pong of ROUNDS rounds between neighbours at four payload sizes (8 B, 4 KiB, a
    multi-workgroup fused size, one above the fused limit): the consumer reads its whole
    target on the GPU BEFORE it waits, so its caches hold the old round, waits with
    shmem_signal_wait_until(GE, r), reads the whole target on the GPU again and requires
    every word to equal r, then answers with its own put_signal;
  * wait_until_all / _any / _some and their vector forms over one signal per PE with a
    status mask, each PE signalling every other, with no barrier in between;
  * the test forms unsatisfied before a barrier-ordered signal and satisfied after it;
  * short ivars at 2-byte offsets, ivars in the host heap with self-PE signalling.

SHMEMX_P2P_TIMEOUT bounds every wait: a lost signal ends the job with a message.  Prints one
line per PE, exit 0 = OK.
"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sos_amd import _lib as L  # noqa: E402
from sos_amd import shmem as S  # noqa: E402
from tests import readback as R  # noqa: E402

ROUNDS = 50
SIZES = (8, 4096, 64 << 10, 2 << 20)   # with SHMEMX_PUT_SIGNAL_FUSED_MAX=1M: three fused, one composed
SET, ADD = 0, 1
EQ, NE, GT, GE, LT, LE = 1, 2, 3, 4, 5, 6
SIZE_MAX = 2**64 - 1
SIGNED = {"short", "int", "long", "longlong", "int32", "int64", "ptrdiff"}
NAMES = open(os.path.join(ROOT, "tests", "golden", "signal_symbols.txt")).read().split()


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    right, left = (me + 1) % P, (me - 1) % P
    stream = S.shmemx_get_stream()
    lib_stream = torch.cuda.ExternalStream(stream)
    bad, checks, called = [], 0, set()

    def expect(want, got, what):
        nonlocal checks
        checks += 1
        if want != got:
            bad.append((what, "want", want, "got", got))

    def dev(nbytes):
        p = S.shmemx_malloc_device(nbytes)
        assert p
        return p

    def zero(p, nbytes):
        S.shmem_putmem(p, bytes(nbytes), nbytes, me)

    # ---- every put_signal form: self and both neighbours ------------------------------------------------
    forms = [n for n in NAMES if "_signal" in n and "put" in n]
    SLOT = 64
    data, sigs = dev(len(forms) * 3 * SLOT), dev(len(forms) * 3 * 8)
    zero(data, len(forms) * 3 * SLOT)
    zero(sigs, len(forms) * 3 * 8)
    S.shmem_barrier_all()
    # k: 0 the PE itself, 1 written by the left neighbour (I write my right's), 2 by the right one
    targets = ((0, me), (1, right), (2, left))

    def elem_size(name):
        m = re.match(r"shmem_(?:(\w+?)_put|put(\d+|mem))_signal", name)
        return ctypes.sizeof(S._BY_VALUE[m.group(1)]) if m.group(1) else (1 if m.group(2) == "mem" else int(m.group(2)) // 8)

    def pattern(i, sender, k, nbytes):
        return ((np.arange(nbytes) + 7 * i + 13 * sender + k) & 0xFF).astype(np.uint8)

    keep = []
    for i, name in enumerate(forms):
        es = elem_size(name)
        nbytes = 3 * es
        for k, pe in targets:
            src = pattern(i, me, k, nbytes)
            if i % 2:   # a device source (the fused launch), else pageable memory (composed)
                src = torch.from_numpy(src).cuda()
                torch.cuda.synchronize()
                sp = src.data_ptr()
            else:
                sp = src.ctypes.data
            keep.append(src)
            getattr(S, name)(data + (3 * i + k) * SLOT, sp, 3, sigs + (3 * i + k) * 8, 1000 * i + k + 1,
                             ADD if i % 4 < 2 else SET, pe)
        called.add(name)
    S.shmem_quiet()
    S.shmem_barrier_all()
    got_d, got_s = R.device_bytes(data, len(forms) * 3 * SLOT), R.device_bytes(sigs, len(forms) * 3 * 8).view(np.uint64)
    for i, name in enumerate(forms):
        nbytes = 3 * elem_size(name)
        for k, sender in ((0, me), (1, left), (2, right)):
            slot = got_d[(3 * i + k) * SLOT:(3 * i + k + 1) * SLOT]
            want = np.zeros(SLOT, np.uint8)
            want[:nbytes] = pattern(i, sender, k, nbytes)
            expect(True, bool(np.array_equal(slot, want)), (name, "payload", k))
            expect(1000 * i + k + 1, int(got_s[3 * i + k]), (name, "signal", k))
    S.shmem_barrier_all()

    # ---- the signal operations --------------------------------------------------------------------------------
    so = dev(64)
    zero(so, 64)
    S.shmem_barrier_all()
    for k, pe in targets:
        S.shmemx_signal_set(so + 8 * k, 40 + k, pe)
        S.shmemx_signal_add(so + 8 * k, 2, pe)
    called |= {"shmemx_signal_set", "shmemx_signal_add"}
    for k in range(3):   # no barrier: the neighbours' updates are waited for
        expect(42 + k, S.shmem_signal_wait_until(so + 8 * k, EQ, 42 + k), ("signal_wait_until", k))
        expect(42 + k, S.shmem_signal_fetch(so + 8 * k), ("signal_fetch", k))
    called |= {"shmem_signal_wait_until", "shmem_signal_fetch"}
    S.shmem_barrier_all()

    # ---- every wait / test form on ivars the neighbours wrote ---------------------------------------------
    sync_forms = [n for n in NAMES if n not in called]
    types = sorted({re.match(r"shmem_(\w+?)_(wait|test)", n).group(1) for n in sync_forms if re.match(r"shmem_\w+?_(wait|test)", n)})
    iv = {}
    for ti, ty in enumerate(types):
        ct = S._BY_VALUE[ty]
        bits = 8 * ctypes.sizeof(ct)
        base = dev(64)
        zero(base, 64)
        # values at the sign boundary: negative for the signed types, above the signed range for the others
        vals = [-(100 * (j + 1) + ti) if ty in SIGNED else (1 << bits) - 1 - (100 * j + ti) for j in range(4)]
        iv[ty] = (base, ct, vals)
    S.shmem_barrier_all()
    for ty, (base, ct, vals) in iv.items():
        es = ctypes.sizeof(ct)
        put = getattr(S, f"shmem_{ty}_p")
        put(base, vals[0], me)
        put(base + es, vals[1], right)
        put(base + 2 * es, vals[2], left)
        put(base + 3 * es, vals[3], me)
    S.shmem_barrier_all()   # the tests among the forms run ONE probe: the values are there
    long_iv = iv["long"][0]
    for name in sync_forms:
        if name in ("shmem_wait", "shmem_wait_until"):
            base, ct, vals = iv["long"]
            (S.shmem_wait(base + 8, 0) if name == "shmem_wait" else S.shmem_wait_until(base + 8, LT, 0))
            expect(vals[1], R.device_bytes(base + 8, 8).view(np.int64)[0], name)
            called.add(name)
            continue
        m = re.fullmatch(r"shmem_(\w+?)_(?:(wait_until|test)(?:_(all|any|some))?(_vector)?|(wait))", name)
        ty = m.group(1)
        base, ct, vals = iv[ty]
        es, signed = ctypes.sizeof(ct), ty in SIGNED
        fn = getattr(S, name)
        far = LT if signed else GT            # every value is beyond this bound ...
        bound = -50 if signed else 1 << (8 * es - 1)   # ... only when compared at the type's width and sign
        status = (ctypes.c_int * 4)(0, 0, 1, 0)       # element 2 is masked
        values = (ct * 4)(*vals)
        indices = (ctypes.c_size_t * 4)(9, 9, 9, 9)
        if m.group(5):
            fn(base + es, 0)   # until it differs from 0: the left neighbour's put
            expect(vals[1], int(np.frombuffer(R.device_bytes(base + es, es).tobytes(), ct)[0]), name)
        elif m.group(3) is None:
            r = fn(base + es, far, bound)
            expect(None if m.group(2) == "wait_until" else 1, r, name)
        else:
            kind, vec = m.group(3), bool(m.group(4))
            # scalar: every unmasked ivar is beyond the bound; vector: equal to its own value
            tail = [status, EQ, values] if vec else [status, far, bound]
            if kind == "some":
                r = fn(base, 4, indices, *tail)
                expect((3, [0, 1, 3]), (r, list(indices)[:3]), name)
            elif kind == "any":
                r = fn(base + es, 3, (ctypes.c_int * 3)(0, 1, 0), EQ if vec else far, (ct * 3)(*vals[1:]) if vec else bound)
                expect(0, r, name)   # the lowest satisfied unmasked index
            else:
                r = fn(base, 4, *tail)
                expect(None if m.group(2) == "wait_until" else 1, r, name)
        called.add(name)
    expect([], sorted(set(NAMES) - called), "every generated form was called")
    # nelems 0 and everything masked: SOS's return values, at once
    expect(SIZE_MAX, S.shmem_long_wait_until_any(long_iv, 0, None, EQ, 1), "wait_until_any nelems 0")
    expect(0, S.shmem_long_wait_until_some(long_iv, 4, (ctypes.c_size_t * 4)(), (ctypes.c_int * 4)(1, 1, 1, 1), EQ, 1),
           "wait_until_some all masked")
    expect(SIZE_MAX, S.shmem_long_test_any(long_iv, 4, (ctypes.c_int * 4)(1, 1, 1, 1), NE, 12345), "test_any all masked")
    expect(1, S.shmem_long_test_all(long_iv, 0, None, EQ, 1), "test_all nelems 0")
    S.shmem_barrier_all()

    # ---- one signal per PE, each PE signalling every other: the _all / _any / _some waits ---------------
    sa = dev(8 * P)
    zero(sa, 8 * P)
    S.shmem_barrier_all()
    for q in range(P):
        S.shmemx_signal_add(sa + 8 * me, me + 1, q)
    mask = [1 if P >= 3 and j == left else 0 for j in range(P)]
    status = (ctypes.c_int * P)(*mask)
    live = [j for j in range(P) if not mask[j]]
    ones = (ctypes.c_uint64 * P)(*[j + 1 for j in range(P)])
    r = S.shmem_uint64_wait_until_any(sa, P, status, GE, 1)
    expect(True, r in live, ("wait_until_any index", r))
    idx = (ctypes.c_size_t * P)()
    r = S.shmem_uint64_wait_until_some_vector(sa, P, idx, status, EQ, ones)
    got = list(idx)[:r]
    expect(True, 1 <= r <= len(live) and got == sorted(got) and set(got) <= set(live), ("wait_until_some_vector", r, got))
    S.shmem_uint64_wait_until_all_vector(sa, P, status, EQ, ones)
    S.shmem_uint64_wait_until_all(sa, P, status, GE, 1)
    words = R.device_bytes(sa, 8 * P).view(np.uint64)
    expect([j + 1 for j in live], [int(words[j]) for j in live], "every unmasked PE's signal after wait_until_all")
    r = S.shmem_uint64_wait_until_some(sa, P, idx, status, NE, 0)
    expect((len(live), live), (r, list(idx)[:r]), "wait_until_some after all arrived")
    expect(live[0], S.shmem_uint64_wait_until_any_vector(sa, P, status, EQ, ones), "wait_until_any_vector lowest index")
    S.shmem_barrier_all()

    # ---- tests: unsatisfied before a barrier-ordered signal, satisfied after it -----------------------------
    sb = dev(8 * P)
    zero(sb, 8 * P)
    S.shmem_barrier_all()
    none = (ctypes.c_int * P)()
    expect(0, S.shmem_uint64_test(sb + 8 * left, EQ, 1), "test before the signal")
    expect(0, S.shmem_uint64_test_all(sb, P, none, NE, 0), "test_all before")
    expect(SIZE_MAX, S.shmem_uint64_test_any(sb, P, none, NE, 0), "test_any before")
    expect(0, S.shmem_uint64_test_some(sb, P, idx, none, NE, 0), "test_some before")
    S.shmem_barrier_all()
    S.shmemx_signal_set(sb + 8 * me, 1, right)
    S.shmem_quiet()
    S.shmem_barrier_all()
    expect(1, S.shmem_uint64_test(sb + 8 * left, EQ, 1), "test after the signal")
    expect(left, S.shmem_uint64_test_any(sb, P, none, NE, 0), "test_any after")
    expect((1, left), (S.shmem_uint64_test_some(sb, P, idx, none, NE, 0), idx[0]), "test_some after")
    expect(1 if P == 1 else 0, S.shmem_uint64_test_all(sb, P, none, NE, 0), "test_all after: one of P set")
    S.shmem_barrier_all()

    # ---- short ivars at 2-byte offsets, waited for without a barrier ------------------------------------------
    sh = dev(64)
    zero(sh, 64)
    S.shmem_barrier_all()
    S.shmem_short_p(sh + 2, -7, right)
    S.shmem_ushort_p(sh + 6, 65535, right)
    S.shmem_short_wait_until(sh + 2, EQ, -7)
    S.shmem_short_wait_until(sh + 2, LT, 0)       # -7 is not 65529
    S.shmem_ushort_wait_until(sh + 6, GT, 65000)
    expect([0, -7, 0, -1], [int(v) for v in R.device_bytes(sh, 8).view(np.int16)], "short ivars and their neighbours")
    expect(0, S.shmem_short_test(sh + 2, GT, 0), "short -1 .. not above 0")
    S.shmem_barrier_all()

    # ---- ivars in the host heap, signalled by the PE itself -----------------------------------------------------
    hw = S.shmem_calloc(16, 8)
    src8 = np.full(1, 0x0123456789ABCDEF, np.uint64)
    S.shmem_long_p(hw, 5, me)
    S.shmem_long_wait_until(hw, EQ, 5)
    S.shmemx_signal_add(hw + 8, 3, me)
    expect(3, S.shmem_signal_wait_until(hw + 8, GE, 3), "host heap signal_wait_until")
    S.shmem_putmem_signal_nbi(hw + 16, src8.ctypes.data, 8, hw + 32, 9, SET, me)
    expect(9, S.shmem_signal_wait_until(hw + 32, EQ, 9), "host heap put_signal_nbi signal")
    expect(0x0123456789ABCDEF, ctypes.c_uint64.from_address(hw + 16).value, "host heap put_signal_nbi payload")
    expect(0, S.shmem_long_test(hw, NE, 5), "host heap test")
    expect(9, S.shmem_signal_fetch(hw + 32), "host heap signal_fetch")
    S.shmem_barrier_all()

    # ---- ping-pong ----------------------------------------------------------------------------------------------
    nmax = max(SIZES)
    target, psig = dev(nmax), dev(8 * len(SIZES))
    zero(target, nmax)
    zero(psig, 8 * len(SIZES))
    with torch.cuda.stream(lib_stream):   # fills run on the library stream, in order with the puts
        src = torch.zeros(nmax // 8, dtype=torch.int64, device="cuda")
        exp = torch.zeros(nmax // 8, dtype=torch.int64, device="cuda")
    S.shmem_barrier_all()
    pairs = [(0, 0)] if P == 1 else [(a, (a + 1) % P) for a in range(P)]

    def send(si, n, r, pe):
        with torch.cuda.stream(lib_stream):
            src[:n // 8].fill_(r)
        S.shmem_putmem_signal_nbi(target, src.data_ptr(), n, psig + 8 * si, 1 if si % 2 else r, ADD if si % 2 else SET, pe)

    def receive(si, n, r):
        L.count_mismatch(exp.data_ptr(), target, n // 8, 8, stream)   # the old round into this PE's caches
        got = S.shmem_signal_wait_until(psig + 8 * si, GE, r)
        expect(r, got, ("ping-pong signal", n, r))
        with torch.cuda.stream(lib_stream):
            exp[:n // 8].fill_(r)
        expect(0, L.count_mismatch(exp.data_ptr(), target, n // 8, 8, stream), ("ping-pong payload words != r", n, r))

    for a, b in pairs:
        for si, n in enumerate(SIZES):
            if me in (a, b):
                S.shmemx_signal_set(psig + 8 * si, 0, me)
                with torch.cuda.stream(lib_stream):
                    exp.fill_(0)
                zero(target, n)
            S.shmem_barrier_all()
            for r in range(1, ROUNDS + 1):
                if a == b:
                    send(si, n, r, me)
                    receive(si, n, r)
                elif me == a:
                    send(si, n, r, b)
                    receive(si, n, r)
                elif me == b:
                    receive(si, n, r)
                    send(si, n, r, a)
            if me in (a, b):
                S.shmem_quiet()
                expect(ROUNDS, S.shmem_signal_fetch(psig + 8 * si), ("signal_fetch after the ping-pong", n))
            S.shmem_barrier_all()

    fused, composed, probes = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    S.sosx_signal_stats(ctypes.byref(fused), ctypes.byref(composed), ctypes.byref(probes))
    expect(True, fused.value > 0 and composed.value > 0, ("fused and composed calls", fused.value, composed.value))
    a_, r_, u_ = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    L.lib().sosx_acquire_stats(ctypes.byref(a_), ctypes.byref(r_), ctypes.byref(u_), None)
    if u_.value:
        bad.append(("unacquired peer reads", u_.value))
    S.shmem_barrier_all()
    sig = {1: "stream", 0: "host"}.get(L.lib().sosx_p2p_signal_mode(), "none")
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} checks OK (p2p signal {sig}, fused {fused.value}, composed {composed.value}, "
          f"probes {probes.value}, {u_.value} unacquired)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
