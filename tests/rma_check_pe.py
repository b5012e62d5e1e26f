"""Multi-PE correctness run of the one-sided family (one process per PE, tools/oshrun, p2p
transport): shmem_<T>_put / get / put_nbi / p / g / iput / iget, shmemx_<T>_ibput / ibget
and shmem_ptr between each PE and its neighbours (me + 1) % n and (me - 1) % n, and the
self-PE form of each, on device-heap remote sides with the local side in device memory,
pinned host memory and pageable host memory; then the strided and block forms with the
calling PE as the target and the symmetric side on the HOST heap.

Every expected byte comes from numpy index arithmetic over bytes regenerated from a seed
(a put is a byte move).  The target is filled with a canary before each call and compared
whole: the bytes a call must not touch keep the canary.  One case runs team reductions on
the bytes a peer has just put, after the barrier: the library's own next launch must see
them.  At the end the library's count of peer reads that followed a wait without an
acquire (sosx_acquire_stats) must be 0.

Prints one line per PE, exit 0 = OK.
"""
import ctypes
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sos_amd import _lib as L  # noqa: E402
from sos_amd import shmem as S  # noqa: E402
from tests import readback as R  # noqa: E402

TYPES = {"char": 1, "short": 2, "float": 4, "double": 8, "longdouble": 16, "size": 8}
NP_TYPE = {"char": np.int8, "short": np.int16, "float": np.float32, "double": np.float64,
           "longdouble": np.longdouble, "size": np.uint64}
CANARY = 0x6B
TAIL = 64
BIG = 64 << 10                      # elements of the largest contiguous call
HEAP = BIG * 16 + TAIL              # bytes of each symmetric buffer
STRIDES = [(1, 1), (3, 1), (1, 5), (2, 3)]
# (type, bsize, nblocks, tst, sst, target byte offset, source byte offset): one per kernel regime
BLOCK_SHAPES = [("float", 100, 30, 128, 256, 8, 8),     # congruent, head and tail
                ("float", 100, 30, 128, 101, 0, 4),     # incongruent, unaligned 16-B loads
                ("short", 40, 30, 64, 64, 2, 0),        # incongruent, 2-B accesses
                ("float", 3, 700, 5, 7, 4, 12),         # small blocks, more than one lane per block
                ("longdouble", 2, 50, 3, 4, 0, 0)]      # 16-B elements


def pattern(tag, pe, nbytes):
    seed = zlib.crc32(f"{tag}/{pe}".encode())
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def acquire_stats():
    a, r, u = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    L.lib().sosx_acquire_stats(ctypes.byref(a), ctypes.byref(r), ctypes.byref(u), None)
    return a.value, r.value, u.value


class Local:
    """A local (non-symmetric, except 'pinned': the host heap) operand of `nbytes` bytes in
    device memory, pinned host memory or pageable host memory."""

    def __init__(self, kind, data, pinned_base):
        self.kind, self.n = kind, data.size
        if kind == "device":
            self.t = torch.from_numpy(data.copy()).cuda() if data.size else torch.empty(16, dtype=torch.uint8,
                                                                                        device="cuda")
            torch.cuda.synchronize()
            self.ptr = self.t.data_ptr()
        elif kind == "pinned":
            self.ptr = pinned_base
            ctypes.memmove(self.ptr, data.ctypes.data, data.size)
        else:
            self.a = data.copy() if data.size else np.zeros(16, np.uint8)
            self.ptr = self.a.ctypes.data

    def bytes(self):
        if self.kind == "device":
            return R.device_bytes(self.ptr, self.n)
        if self.kind == "pinned":
            return np.frombuffer(ctypes.string_at(self.ptr, self.n), np.uint8)
        return self.a[:self.n].copy()


def blocks(buf, off, es, bsize, nblocks, stride):
    """(nblocks, bsize * es) byte view of the blocks `stride` elements apart from byte `off`."""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(nblocks, bsize * es), strides=(stride * es, 1))


def extent(es, bsize, nblocks, stride):
    return ((nblocks - 1) * stride + bsize) * es if nblocks and bsize else 0


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    world = S.team_world()
    right, left = (me + 1) % P, (me - 1) % P
    bad, checks = [], 0
    tgt = S.shmemx_malloc_device(HEAP)     # what peers put into / the self-PE target
    src = S.shmemx_malloc_device(HEAP)     # what peers get from
    red = S.shmemx_malloc_device(HEAP)     # the reduction's result
    pinned = S.shmem_malloc(HEAP)          # host symmetric heap: a pinned local side
    S.shmem_barrier_all()

    def check(exp, got, what):
        nonlocal checks
        checks += 1
        if exp.size != got.size or R.mismatches(exp, got, 1):
            bad.append(what)

    def dev_write(ptr, data):
        if data.size:
            L.check(L.lib().sosx_memcpy(ptr, data.ctypes.data, data.size, None), "sosx_memcpy")

    def fill_target(nbytes):
        dev_write(tgt, np.full(nbytes + TAIL, CANARY, np.uint8))

    # ---- put, get, put_nbi: every type, sizes 0, 1, V + 1, 64 Ki; the local side rotates ------
    kinds = ("device", "pinned", "pageable")
    k = 0
    for ty, es in TYPES.items():
        put, get = getattr(S, f"shmem_{ty}_put"), getattr(S, f"shmem_{ty}_get")
        put_nbi = getattr(S, f"shmem_{ty}_put_nbi")
        for n in (0, 1, 16 // es + 1, BIG):
            for kind in (kinds if ty == "float" else (kinds[k % 3],)):
                k += 1
                tag, nb = f"put/{ty}/{n}/{kind}", n * es
                for pe, frm in ((right, left), (me, me)):   # the neighbour, then the calling PE itself
                    fill_target(nb)
                    dev_write(src, pattern(tag + "/get", me, nb))
                    S.shmem_barrier_all()
                    loc = Local(kind, pattern(tag, me, nb), pinned)
                    put(tgt, loc.ptr, n, pe)
                    S.shmem_barrier_all()
                    exp = np.concatenate([pattern(tag, frm, nb), np.full(TAIL, CANARY, np.uint8)])
                    check(exp, R.device_bytes(tgt, nb + TAIL), (tag, "pe", pe))
                    # get what PE `pe` holds in src
                    out = Local(kind, np.full(nb + TAIL, CANARY, np.uint8), pinned)
                    get(out.ptr, src, n, pe)
                    exp = np.concatenate([pattern(tag + "/get", pe, nb), np.full(TAIL, CANARY, np.uint8)])
                    check(exp, out.bytes(), (tag, "get", pe))
                    S.shmem_barrier_all()
            # four nbi puts of a quarter each (ragged), then quiet and a barrier
            fill_target(n * es)
            S.shmem_barrier_all()
            loc = Local("device", pattern(f"nbi/{ty}/{n}", me, n * es), pinned)
            cuts = [0, n // 4, n // 2, n - n // 4, n]
            for a, b in zip(cuts, cuts[1:]):
                put_nbi(tgt + a * es, loc.ptr + a * es, b - a, right)
            S.shmem_quiet()
            S.shmem_barrier_all()
            exp = np.concatenate([pattern(f"nbi/{ty}/{n}", left, n * es), np.full(TAIL, CANARY, np.uint8)])
            check(exp, R.device_bytes(tgt, n * es + TAIL), ("put_nbi", ty, n))
        # get_nbi + quiet
        n = 1000
        dev_write(src, pattern(f"gnbi/{ty}", me, n * es))
        S.shmem_barrier_all()
        out = Local("device", np.full(n * es, CANARY, np.uint8), pinned)
        getattr(S, f"shmem_{ty}_get_nbi")(out.ptr, src, n, right)
        S.shmem_quiet()
        check(pattern(f"gnbi/{ty}", right, n * es), out.bytes(), ("get_nbi", ty))
        S.shmem_barrier_all()
        # p / g round trip: element 3 of the right neighbour's target, then read it back
        val = 7 * (me + 1) + 1
        arg = bytes([val]) if ty == "char" else (float(val) if ty in ("float", "double", "longdouble") else val)
        fill_target(8 * es)
        S.shmem_barrier_all()
        getattr(S, f"shmem_{ty}_p")(tgt + 3 * es, arg, right)
        S.shmem_barrier_all()
        got = R.device_bytes(tgt, 8 * es + TAIL)
        mine = np.frombuffer(got[3 * es:4 * es].tobytes(), NP_TYPE[ty])[0]
        checks += 2
        if float(mine) != float(7 * (left + 1) + 1) or (np.delete(got, range(3 * es, 4 * es)) != CANARY).any():
            bad.append(("p", ty, float(mine)))
        back = getattr(S, f"shmem_{ty}_g")(tgt + 3 * es, right)
        back = back[0] if ty == "char" else back
        if float(back) != float(val):
            bad.append(("g", ty, float(back)))
        S.shmem_barrier_all()

    # ---- iput / iget -----------------------------------------------------------------------
    for ty in ("char", "float", "longdouble"):
        es = TYPES[ty]
        iput, iget = getattr(S, f"shmem_{ty}_iput"), getattr(S, f"shmem_{ty}_iget")
        for tst, sst in STRIDES:
            for n in (16 // es + 1, 1500):
                for kind in (("device", "pageable") if n == 1500 else ("pinned",)):
                    tag = f"iput/{ty}/{tst}/{sst}/{n}/{kind}"
                    text, sext = extent(es, 1, n, tst), extent(es, 1, n, sst)
                    for pe, frm in ((right, left), (me, me)):
                        fill_target(text)
                        dev_write(src, pattern(tag + "/get", me, sext))
                        S.shmem_barrier_all()
                        loc = Local(kind, pattern(tag, me, sext), pinned)
                        iput(tgt, loc.ptr, tst, sst, n, pe)
                        S.shmem_barrier_all()
                        exp = np.full(text + TAIL, CANARY, np.uint8)
                        blocks(exp, 0, es, 1, n, tst)[:] = blocks(pattern(tag, frm, sext), 0, es, 1, n, sst)
                        check(exp, R.device_bytes(tgt, text + TAIL), (tag, "pe", pe))
                        # iget: source stride sst on PE pe's src, target stride tst here
                        out = Local(kind, np.full(text + TAIL, CANARY, np.uint8), pinned)
                        iget(out.ptr, src, tst, sst, n, pe)
                        exp = np.full(text + TAIL, CANARY, np.uint8)
                        blocks(exp, 0, es, 1, n, tst)[:] = blocks(pattern(tag + "/get", pe, sext), 0, es, 1, n, sst)
                        check(exp, out.bytes(), (tag, "iget", pe))
                        S.shmem_barrier_all()

    # ---- ibput / ibget: one shape from each kernel regime --------------------------------------
    for ty, bsize, nblocks, tst, sst, toff, soff in BLOCK_SHAPES:
        es = TYPES[ty]
        ibput, ibget = getattr(S, f"shmemx_{ty}_ibput"), getattr(S, f"shmemx_{ty}_ibget")
        text, sext = extent(es, bsize, nblocks, tst), extent(es, bsize, nblocks, sst)
        for kind in kinds:
            tag = f"ibput/{ty}/{bsize}/{nblocks}/{tst}/{sst}/{kind}"
            for pe, frm in ((right, left), (me, me)):
                fill_target(toff + text)
                dev_write(src, pattern(tag + "/get", me, soff + sext))
                S.shmem_barrier_all()
                loc = Local(kind, pattern(tag, me, soff + sext), pinned)
                ibput(tgt + toff, loc.ptr + soff, tst, sst, bsize, nblocks, pe)
                S.shmem_barrier_all()
                exp = np.full(toff + text + TAIL, CANARY, np.uint8)
                blocks(exp, toff, es, bsize, nblocks, tst)[:] = \
                    blocks(pattern(tag, frm, soff + sext), soff, es, bsize, nblocks, sst)
                check(exp, R.device_bytes(tgt, toff + text + TAIL), (tag, "pe", pe))
                out = Local(kind, np.full(toff + text + TAIL, CANARY, np.uint8), pinned)
                ibget(out.ptr + toff, src + soff, tst, sst, bsize, nblocks, pe)
                exp = np.full(toff + text + TAIL, CANARY, np.uint8)
                blocks(exp, toff, es, bsize, nblocks, tst)[:] = \
                    blocks(pattern(tag + "/get", pe, soff + sext), soff, es, bsize, nblocks, sst)
                check(exp, out.bytes(), (tag, "ibget", pe))
                S.shmem_barrier_all()

    # ---- the calling PE itself with the symmetric side on the HOST heap ---------------------------
    # (pe == my_pe takes any symmetric memory; static data: tests/rma_static_pe.c)
    hsym = S.shmem_malloc(HEAP)

    def host_bytes(n):
        return np.frombuffer(ctypes.string_at(hsym, n), np.uint8)

    host_shapes = BLOCK_SHAPES + [("float", 1, 1500, t, s_, 0, 0) for t, s_ in STRIDES]
    for ty, bsize, nblocks, tst, sst, toff, soff in host_shapes:
        es = TYPES[ty]
        strided = bsize == 1 and (ty, bsize, nblocks, tst, sst, toff, soff) not in BLOCK_SHAPES
        text, sext = extent(es, bsize, nblocks, tst), extent(es, bsize, nblocks, sst)
        for kind in kinds:
            tag = f"hostheap/{ty}/{bsize}/{nblocks}/{tst}/{sst}/{kind}"
            ctypes.memset(hsym, CANARY, toff + text + TAIL)
            loc = Local(kind, pattern(tag, me, soff + sext), pinned)
            if strided:
                getattr(S, f"shmem_{ty}_iput")(hsym + toff, loc.ptr + soff, tst, sst, nblocks, me)
            else:
                getattr(S, f"shmemx_{ty}_ibput")(hsym + toff, loc.ptr + soff, tst, sst, bsize, nblocks, me)
            exp = np.full(toff + text + TAIL, CANARY, np.uint8)
            blocks(exp, toff, es, bsize, nblocks, tst)[:] = \
                blocks(pattern(tag, me, soff + sext), soff, es, bsize, nblocks, sst)
            check(exp, host_bytes(toff + text + TAIL), (tag, "put"))
            data = pattern(tag + "/get", me, soff + sext)
            ctypes.memmove(hsym, data.ctypes.data, data.size)
            out = Local(kind, np.full(toff + text + TAIL, CANARY, np.uint8), pinned)
            if strided:
                getattr(S, f"shmem_{ty}_iget")(out.ptr + toff, hsym + soff, tst, sst, nblocks, me)
            else:
                getattr(S, f"shmemx_{ty}_ibget")(out.ptr + toff, hsym + soff, tst, sst, bsize, nblocks, me)
            exp = np.full(toff + text + TAIL, CANARY, np.uint8)
            blocks(exp, toff, es, bsize, nblocks, tst)[:] = blocks(data, soff, es, bsize, nblocks, sst)
            check(exp, out.bytes(), (tag, "get"))
    S.shmem_barrier_all()
    S.shmem_free(hsym)

    # ---- shmem_ptr ---------------------------------------------------------------------------
    dev_write(src, pattern("ptr", me, 4096))
    S.shmem_barrier_all()
    checks += 3
    if S.shmem_ptr(src, me) != src:
        bad.append(("shmem_ptr", "self"))
    if S.shmem_ptr(pinned, me) != pinned:
        bad.append(("shmem_ptr", "self host heap"))
    if P > 1:
        p = S.shmem_ptr(src + 256, right)
        if not p or p == src + 256:
            bad.append(("shmem_ptr", "peer is NULL or untranslated", p))
        else:
            check(pattern("ptr", right, 4096)[256:], R.device_bytes(p, 4096 - 256), ("shmem_ptr", "peer bytes"))
        if S.shmem_ptr(pinned, right) is not None:
            bad.append(("shmem_ptr", "peer host heap is not NULL"))
    S.shmem_barrier_all()

    # ---- the library's next launch sees what a peer put: reductions on the put bytes ------------
    n = 20000
    for rep in range(3):
        vals = [np.random.default_rng(1000 * rep + q).integers(-1000, 1000, n, dtype=np.int32) for q in range(P)]
        S.shmem_int_put(tgt, vals[me].ctypes.data, n, right)   # pageable source
        S.shmem_barrier_all()
        S.shmem_int_sum_reduce(world, red, tgt, n)             # every PE's tgt holds its left neighbour's
        want = sum(v.astype(np.int64) for v in vals).astype(np.int32)
        check(want.view(np.uint8), R.device_bytes(red, 4 * n), ("reduce after put", rep))
        S.shmem_barrier_all()

    acq, reads, unacq = acquire_stats()
    if unacq:
        bad.append(("unacquired peer reads", unacq))
    S.shmem_barrier_all()
    S.shmem_free(pinned)
    for p in (red, src, tgt):
        S.shmemx_free_device(p)
    sig = {1: "stream", 0: "host"}.get(L.lib().sosx_p2p_signal_mode(), "none")
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} checks OK (p2p signal {sig}, peer reads {reads}, {unacq} unacquired)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
