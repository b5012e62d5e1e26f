"""Multi-PE correctness run of the communication contexts (one process per PE, tools/oshrun,
p2p transport).  Every expected value is computed here with numpy, never by the library.

  families    each one-sided family through a created context next to the same call on the
              default context: put / get at 1, 2, 8 and 16-byte elements and counts 1, 3, 1025,
              65537; iput / iget (2 and 8 bytes) and ibput / ibget (1 and 16 bytes) at the
              same counts; p / g; fetch_add, compare_swap, swap and fetch_or; a fetching nbi
              atomic filled by the context's quiet; put with signal (fused, and composed above
              SHMEMX_PUT_SIGNAL_FUSED_MAX) awaited with shmem_signal_wait_until; a context on a
              strided team (index 1 lands on the right world PE and nowhere else,
              shmem_ctx_get_team); shmem_team_destroy delivering a pending put_nbi; and
              shmem_finalize with a live context.  Canaries either side of every target.
  completion  (test build of the library: sosx_ctx_stats) two contexts A and B, a put_nbi on
              each: shmem_ctx_quiet(A) completes A alone, shmem_quiet touches neither.

Prints one line per PE, exit 0 = OK.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sos_amd import _lib as L  # noqa: E402
from sos_amd import shmem as S  # noqa: E402
from tests import readback as R  # noqa: E402

CAN = 64            # canary bytes either side of a target
FILL = 0xEE
COUNTS = (1, 3, 1025, 65537)
TYPES = (("char", 1), ("short", 2), ("double", 8), ("longdouble", 16))
SET, EQ = 0, 1


def pattern(pe, case, nbytes):
    return ((np.arange(nbytes, dtype=np.int64) * 31 + 7 * pe + 3 * case) & 0xFF).astype(np.uint8)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "families"
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    right, left = (me + 1) % P, (me - 1) % P
    bad, checks = [], 0

    def expect(want, got, what):
        nonlocal checks
        checks += 1
        if isinstance(want, np.ndarray):
            ok = want.shape == got.shape and bool(np.array_equal(want, got))
            if not ok:
                bad.append((what, "first difference at", int(np.flatnonzero(want != got)[0]) if want.shape == got.shape else -1))
        elif want != got:
            bad.append((what, "want", want, "got", got))

    def dev(nbytes, fill=None):
        p = S.shmemx_malloc_device(nbytes)
        assert p
        if fill is not None:
            src = np.full(nbytes, fill, np.uint8) if np.isscalar(fill) else fill
            S.shmem_putmem(p, src.ctypes.data, nbytes, me)
        return p

    def refill(p, nbytes):
        src = np.full(nbytes, FILL, np.uint8)   # held until the blocking put returns
        S.shmem_putmem(p, src.ctypes.data, nbytes, me)

    def framed(payload, total):
        """What a target of `total` bytes holds: canary, payload, canary to the end."""
        out = np.full(total, FILL, np.uint8)
        out[CAN:CAN + payload.size] = payload
        return out

    def new_ctx(options=0):
        h = ctypes.c_void_p()
        expect(0, S.shmem_ctx_create(options, ctypes.byref(h)), "shmem_ctx_create")
        return h.value

    def stats(ctx):
        out = (ctypes.c_longlong * 6)()
        f = L.lib().sosx_ctx_stats
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
        f(ctx, out)
        return dict(zip(("stream", "slot", "enqueued", "completed", "releases", "syncs"), out))

    if mode == "completion":
        n, case = 1025 * 8, 99
        src_a, src_b = dev(n, pattern(me, case, n)), dev(n, pattern(me, case + 1, n))
        dst_a, dst_b = dev(n + 2 * CAN, FILL), dev(n + 2 * CAN, FILL)
        A, B = new_ctx(), new_ctx()
        S.shmem_barrier_all()
        S.shmem_ctx_putmem_nbi(A, dst_a + CAN, src_a, n, right)
        S.shmem_ctx_putmem_nbi(B, dst_b + CAN, src_b, n, right)
        a0, b0 = stats(A), stats(B)
        expect(True, a0["stream"] != b0["stream"] and a0["slot"] != b0["slot"], ("A and B on different streams", a0, b0))
        expect(True, S.shmemx_get_stream() not in (a0["stream"], b0["stream"]), "neither is the library stream")
        expect((1, 0, 0), (a0["enqueued"], a0["completed"], a0["syncs"]), ("A before its quiet", a0))
        expect((1, 0, 0), (b0["enqueued"], b0["completed"], b0["syncs"]), ("B before A's quiet", b0))
        S.shmem_ctx_quiet(A)
        a1, b1 = stats(A), stats(B)
        expect((1, 1, 1, a0["releases"] + 1), (a1["enqueued"], a1["completed"], a1["syncs"], a1["releases"]),
               ("A's quiet completed A", a1))
        expect(b0, b1, "A's quiet recorded no release on B and did not synchronise B's stream")
        S.shmem_quiet()
        expect((a1, b1), (stats(A), stats(B)), "shmem_quiet touched neither A nor B")
        S.shmem_ctx_quiet(B)
        b2 = stats(B)
        expect((1, 1, 1, b1["releases"] + 1), (b2["enqueued"], b2["completed"], b2["syncs"], b2["releases"]),
               ("B's quiet completed B", b2))
        expect(a1, stats(A), "B's quiet left A alone")
        S.shmem_barrier_all()
        expect(framed(pattern(left, case, n), n + 2 * CAN), R.device_bytes(dst_a, n + 2 * CAN), "A's payload at the neighbour")
        expect(framed(pattern(left, case + 1, n), n + 2 * CAN), R.device_bytes(dst_b, n + 2 * CAN), "B's payload at the neighbour")
        S.shmem_ctx_destroy(A)
        S.shmem_ctx_destroy(B)
        return finish(me, P, bad, checks, "completion")

    # ---- families ------------------------------------------------------------------------------------
    ctx = new_ctx()
    other = new_ctx(S.SHMEM_CTX_SERIALIZED)   # a second one: with SHMEMX_CTX_STREAMS=1 they share a stream
    team = ctypes.c_void_p()
    expect(0, S.shmem_ctx_get_team(ctx, ctypes.byref(team)), "shmem_ctx_get_team(world context)")
    expect(S.team_world(), team.value, "a context of shmem_ctx_create is on the world team")
    expect(-1, S.shmem_ctx_get_team(None, ctypes.byref(team)), "shmem_ctx_get_team(SHMEM_CTX_INVALID)")
    expect(None, team.value, "... sets SHMEM_TEAM_INVALID")
    bogus = ctypes.c_void_p(1)
    expect(True, S.shmem_ctx_create(8, ctypes.byref(bogus)) != 0 and bogus.value is None, "unknown option bits")
    expect(-1, S.shmem_team_create_ctx(None, 0, ctypes.byref(bogus)), "shmem_team_create_ctx(SHMEM_TEAM_INVALID)")
    S.shmem_ctx_destroy(None)  # a no-op
    case = 0
    for tname, es in TYPES:
        for n in COUNTS:
            case += 1
            strided = es in (2, 8)
            bsize = 3
            nblocks = (n + bsize - 1) // bsize
            nsrc = n if strided else nblocks * bsize           # elements the source holds
            span = 2 * n if strided else nblocks * 4           # elements the strided / block target spans
            nb, total = n * es, span * es + 2 * CAN
            src = dev(nsrc * es, pattern(me, case, nsrc * es))
            ta, tb = dev(total, FILL), dev(total, FILL)        # the context's target, the default context's
            ga, gb = dev(total, FILL), dev(total, FILL)        # local targets of the gets
            S.shmem_barrier_all()
            # put / get (put_nbi + the context's quiet for the odd cases)
            if case % 2:
                getattr(S, f"shmem_ctx_{tname}_put_nbi")(other, ta + CAN, src, n, right)
                S.shmem_ctx_quiet(other)
            else:
                getattr(S, f"shmem_ctx_{tname}_put")(ctx, ta + CAN, src, n, right)
            getattr(S, f"shmem_{tname}_put")(tb + CAN, src, n, right)
            getattr(S, f"shmem_ctx_{tname}_get")(ctx, ga + CAN, src, n, right)
            getattr(S, f"shmem_{tname}_get")(gb + CAN, src, n, right)
            S.shmem_barrier_all()
            want = framed(pattern(left, case, nsrc * es)[:nb], total)
            expect(want, R.device_bytes(ta, total), (tname, n, "ctx put"))
            expect(want, R.device_bytes(tb, total), (tname, n, "put"))
            want = framed(pattern(right, case, nsrc * es)[:nb], total)
            expect(want, R.device_bytes(ga, total), (tname, n, "ctx get"))
            expect(want, R.device_bytes(gb, total), (tname, n, "get"))
            for p in (ta, tb, ga, gb):
                refill(p, total)
            S.shmem_barrier_all()
            # iput / iget (target stride 2) or ibput / ibget (blocks of 3, 4 apart)
            if strided:
                put, get, args = f"{tname}_iput", f"{tname}_iget", (2, 1, n)
            else:
                put, get, args = f"{tname}_ibput", f"{tname}_ibget", (4, 3, bsize, nblocks)
            pre = "shmem" if strided else "shmemx"
            getattr(S, f"{pre}_ctx_{put}")(ctx, ta + CAN, src, *args, right)
            getattr(S, f"{pre}_{put}")(tb + CAN, src, *args, right)
            getattr(S, f"{pre}_ctx_{get}")(other, ga + CAN, src, *args, right)
            getattr(S, f"{pre}_{get}")(gb + CAN, src, *args, right)
            S.shmem_barrier_all()

            def spread(sender):
                s = pattern(sender, case, nsrc * es).reshape(-1, es)
                out = np.full((span, es), FILL, np.uint8)
                if strided:
                    out[0:2 * n:2] = s[:n]
                else:
                    out.reshape(nblocks, 4, es)[:, :bsize] = s.reshape(nblocks, bsize, es)
                return framed(out.reshape(-1), total)

            expect(spread(left), R.device_bytes(ta, total), (tname, n, "ctx " + put))
            expect(spread(left), R.device_bytes(tb, total), (tname, n, put))
            expect(spread(right), R.device_bytes(ga, total), (tname, n, "ctx " + get))
            expect(spread(right), R.device_bytes(gb, total), (tname, n, get))
            for p in (gb, ga, tb, ta, src):
                S.shmemx_free_device(p)
    # p / g
    pg = dev(64, FILL)
    vals = dev(32, np.frombuffer(np.array([me + 1.5], np.float64).tobytes() + np.array([me + 11], np.int16).tobytes()
                                 + bytes([me + 21]) + bytes(21), np.uint8).copy())
    S.shmem_barrier_all()
    S.shmem_ctx_double_p(ctx, pg, me + 0.25, right)
    S.shmem_ctx_short_p(ctx, pg + 8, me + 100, right)
    S.shmem_ctx_char_p(other, pg + 10, bytes([me + 65]), right)
    S.shmem_double_p(pg + 16, me + 0.25, right)
    expect(right + 1.5, S.shmem_ctx_double_g(ctx, vals, right), "ctx double g")
    expect(right + 11, S.shmem_ctx_short_g(ctx, vals + 8, right), "ctx short g")
    expect(bytes([right + 21]), S.shmem_ctx_char_g(other, vals + 10, right), "ctx char g")
    expect(right + 1.5, S.shmem_double_g(vals, right), "double g")
    S.shmem_barrier_all()
    got = R.device_bytes(pg, 64)
    want = np.full(64, FILL, np.uint8)
    want[0:8] = np.frombuffer(np.array([left + 0.25], np.float64).tobytes(), np.uint8)
    want[8:10] = np.frombuffer(np.array([left + 100], np.int16).tobytes(), np.uint8)
    want[10] = left + 65
    want[16:24] = want[0:8]
    expect(want, got, "ctx p / p")
    # atomics: words 0..3 through the context, 4..7 through the default context; only the left neighbour
    # touches a PE's words, so every old value is known
    W = dev(64, 0)
    S.shmem_barrier_all()
    for base, c in ((0, ctx), (32, None)):
        f = (lambda n: (lambda *a: getattr(S, f"shmem_ctx_uint64_atomic_{n}")(c, *a))) if c else \
            (lambda n: getattr(S, f"shmem_uint64_atomic_{n}"))
        expect(0, f("fetch_add")(W + base, me + 1, right), ("fetch_add old", base))
        expect(0, f("compare_swap")(W + base + 8, 0, 100 + me, right), ("compare_swap old", base))
        expect(0, f("swap")(W + base + 16, 7 + me, right), ("swap old", base))
        expect(0, f("fetch_or")(W + base + 24, 1 << me, right), ("fetch_or old", base))
        expect(100 + me, f("compare_swap")(W + base + 8, 5, 1, right), ("compare_swap that fails", base))
    # a fetching nbi atomic into pageable memory: filled by the context's quiet
    fetched = np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)
    S.shmem_ctx_uint64_atomic_fetch_add_nbi(ctx, fetched.ctypes.data, W, 5, right)
    S.shmem_uint64_atomic_fetch_add_nbi(fetched.ctypes.data + 8, W + 32, 5, right)
    S.shmem_ctx_quiet(ctx)
    expect(me + 1, int(fetched[0]), "ctx fetch_add_nbi filled by shmem_ctx_quiet")
    S.shmem_quiet()
    expect(me + 1, int(fetched[1]), "fetch_add_nbi filled by shmem_quiet")
    S.shmem_barrier_all()
    want = np.array([left + 6, 100 + left, 7 + left, 1 << left] * 2, np.uint64)
    expect(want, R.device_bytes(W, 64).view(np.uint64), "atomics at the neighbour")
    # put with signal: 3 x 16 bytes fused, 65537 x 16 bytes above SHMEMX_PUT_SIGNAL_FUSED_MAX=1M composed
    fused0, comp0 = ctypes.c_long(), ctypes.c_long()
    S.sosx_signal_stats(ctypes.byref(fused0), ctypes.byref(comp0), None)
    for k, n in enumerate((3, 65537)):
        nb = 16 * n
        src, dst, sig = dev(nb, pattern(me, 200 + k, nb)), dev(nb + 2 * CAN, FILL), dev(8, 0)
        S.shmem_barrier_all()
        if k:
            S.shmem_ctx_put128_signal(other, dst + CAN, src, n, sig, me + 1, SET, right)
        else:
            S.shmem_ctx_put128_signal_nbi(ctx, dst + CAN, src, n, sig, me + 1, SET, right)
            S.shmem_ctx_quiet(ctx)
        expect(left + 1, S.shmem_signal_wait_until(sig, EQ, left + 1), ("signal", n))
        expect(framed(pattern(left, 200 + k, nb), nb + 2 * CAN), R.device_bytes(dst, nb + 2 * CAN), ("ctx put_signal", n))
    fused1, comp1 = ctypes.c_long(), ctypes.c_long()
    S.sosx_signal_stats(ctypes.byref(fused1), ctypes.byref(comp1), None)
    expect((1, 1), (fused1.value - fused0.value, comp1.value - comp0.value), "one fused, one composed")
    uid = dev(16, 0)
    S.shmem_barrier_all()
    S.shmemx_ctx_signal_add(ctx, uid, 3 + me, right)
    S.shmemx_ctx_signal_set(other, uid + 8, 40 + me, right)
    S.shmem_ctx_fence(ctx)
    S.shmem_ctx_fence(other)
    expect(3 + left, S.shmem_signal_wait_until(uid, EQ, 3 + left), "shmemx_ctx_signal_add")
    expect(40 + left, S.shmem_signal_wait_until(uid + 8, EQ, 40 + left), "shmemx_ctx_signal_set")
    # ---- a team context ------------------------------------------------------------------------------
    if P >= 2:
        # 3 PEs: the odd PEs {1} (index 0 is PE 1) and the stride-2 team {0, 2} (index 1 is PE 2);
        # 2 PEs: the stride-1 sub-team {0, 1}
        splits = [(1, 2, 1), (0, 2, 2)] if P >= 3 else [(0, 1, 2)]
        for start, stride, size in splits:
            tgt, tgt2 = dev(256 + 2 * CAN, FILL), dev(256 + 2 * CAN, FILL)
            tsrc = dev(256, pattern(me, 300 + start, 256))
            th = ctypes.c_void_p()
            S.shmem_team_split_strided(S.team_world(), start, stride, size, None, 0, ctypes.byref(th))
            member = th.value is not None
            idx = size - 1                     # the team's last member
            dest_pe = start + idx * stride     # ... as a world PE
            writer = start                     # team index 0 writes
            tctx = ctypes.c_void_p()
            if member:
                expect(0, S.shmem_team_create_ctx(th, 0, ctypes.byref(tctx)), "shmem_team_create_ctx")
                back = ctypes.c_void_p()
                expect(0, S.shmem_ctx_get_team(tctx, ctypes.byref(back)), "shmem_ctx_get_team")
                expect(th.value, back.value, "shmem_ctx_get_team returns the team")
                if me == writer:
                    S.shmem_ctx_putmem(tctx, tgt + CAN, tsrc, 256, idx)
            S.shmem_barrier_all()
            want = framed(pattern(writer, 300 + start, 256), 256 + 2 * CAN) if me == dest_pe else \
                np.full(256 + 2 * CAN, FILL, np.uint8)
            expect(want, R.device_bytes(tgt, 256 + 2 * CAN), ("team context put lands on world PE", dest_pe, "only"))
            # teardown: a put_nbi pending on the team's context is delivered by shmem_team_destroy
            if member:
                if me == writer:
                    S.shmem_ctx_putmem_nbi(tctx, tgt2 + CAN, tsrc, 256, idx)
                S.shmem_team_destroy(th)
            S.shmem_barrier_all()
            expect(want, R.device_bytes(tgt2, 256 + 2 * CAN), ("shmem_team_destroy delivered the pending put", dest_pe))
    S.shmem_ctx_destroy(other)
    # shmem_finalize with a live context and a put_nbi pending on it
    last = dev(64, FILL)
    S.shmem_barrier_all()
    S.shmem_ctx_putmem_nbi(ctx, last, W, 64, right)
    return finish(me, P, bad, checks, "families")


def finish(me, P, bad, checks, mode):
    a_, r_, u_ = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    L.lib().sosx_acquire_stats(ctypes.byref(a_), ctypes.byref(r_), ctypes.byref(u_), None)
    if u_.value:
        bad.append(("unacquired peer reads", u_.value))
    streams = S.sosx_ctx_streams()
    S.shmem_barrier_all()
    sig = {1: "stream", 0: "host"}.get(L.lib().sosx_p2p_signal_mode(), "none")
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} {mode} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} {mode} checks OK (p2p signal {sig}, context streams {streams}, peer reads {r_.value}, "
          f"{u_.value} unacquired)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
