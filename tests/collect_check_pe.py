"""Multi-PE correctness run of fcollect, alltoall and alltoalls (one process per PE).

Run under tools/oshrun: every PE calls shmem_<T>_fcollect, shmem_<T>_alltoall and
shmem_<T>_alltoalls (typed and mem forms) over SHMEM_TEAM_WORLD and an even-PE split
team, and the deprecated 32/64 active-set forms over the world, on device-heap buffers
(shmemx_malloc_device), plain device buffers, pageable host buffers and host
symmetric-heap buffers.  Every member's input is regenerated on the CPU (the oracle's
generator; the oracle has no entry for these collectives) and the PE's own target is
compared with the closed form of SOS's index arithmetic (src/collectives.c:1284-1531):

  fcollect   target = concat over members q of source(q)
  alltoall   target block j = block `me` of source(member j)
  alltoalls  the same blocks, element k of the packed operand at k*sst elements of the
             source and k*dst elements of the target; the bytes between target elements
             keep the sentinel they held before the call.

Prints one line per PE, exit 0 = OK.
"""
import ctypes
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import oracle as O  # noqa: E402
from sos_amd import _lib as L  # noqa: E402
from sos_amd import shmem as S  # noqa: E402
from tests import readback as R  # noqa: E402

TYPES = {"int": 4, "double": 8, "uint8": 1, "longdouble": 16, "mem": 1}
SIZES = [1, 37, 5003]
BIG = (1 << 18) + 3       # int only, heap and device buffers only
STRIDES = [(1, 1), (1, 2), (3, 1), (2, 3)]
MODES = ("heap", "device", "host", "hostheap")
SENTINEL = 0x6B
UCHAR = L.DTYPES["uchar"]


def fill(seed, pe, nbytes):
    return R.as_bytes(O.fill(UCHAR, L.DIST_UNIFORM, seed, pe, nbytes))


def extent(n, stride, es):
    return es * ((n - 1) * stride + 1)


def spread(packed, n, stride, es):
    """The strided operand holding `packed` (n elements): sentinel in the gaps."""
    out = np.full(extent(n, stride, es), SENTINEL, np.uint8)
    np.lib.stride_tricks.as_strided(out, shape=(n, es), strides=(stride * es, 1))[:] = packed.reshape(n, es)
    return out


def memcpy(dst, src, n):
    L.check(L.lib().sosx_memcpy(dst, src, n, None), "sosx_memcpy")


class Buffers:
    def __init__(self, hsrc, hdst, hh):
        self.hsrc, self.hdst, self.hh = hsrc, hdst, hh

    def run(self, mode, src, init, call):
        """Place the source bytes and the target's initial bytes (numpy uint8), call(dst,
        src), return the target's bytes."""
        if mode == "heap":
            memcpy(self.hsrc, src.ctypes.data, src.size)
            memcpy(self.hdst, init.ctypes.data, init.size)
            call(self.hdst, self.hsrc)
            return R.device_bytes(self.hdst, init.size)
        if mode == "device":
            s = torch.from_numpy(src.copy()).cuda()
            d = torch.from_numpy(init.copy()).cuda()
            torch.cuda.synchronize()
            call(d.data_ptr(), s.data_ptr())
            return R.device_bytes(d.data_ptr(), init.size)
        if mode == "hostheap":
            hs, hd = self.hh
            ctypes.memmove(hs, src.ctypes.data, src.size)
            ctypes.memmove(hd, init.ctypes.data, init.size)
            call(hd, hs)
            return np.ctypeslib.as_array((ctypes.c_uint8 * init.size).from_address(hd)).copy()
        h_in, h_out = src.copy(), init.copy()
        call(h_out.ctypes.data, h_in.ctypes.data)
        return h_out


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    world = S.team_world()
    bad, checks = [], 0
    heap_bytes = extent(P * BIG, 3, 4) + 64
    host_bytes = extent(P * max(SIZES), 3, 16) + 64
    hsrc = S.shmemx_malloc_device(heap_bytes)
    hdst = S.shmemx_malloc_device(heap_bytes)
    hh = (S.shmem_malloc(host_bytes), S.shmem_malloc(host_bytes))
    psync = S.shmem_malloc(8 * 64)
    ctypes.memset(psync, 0, 8 * 64)
    S.shmem_barrier_all()
    bufs = Buffers(hsrc, hdst, hh)
    even = ctypes.c_void_p(0)
    if P >= 3:
        S.lib().shmem_team_split_strided(world, 0, 2, (P + 1) // 2, None, 0, ctypes.byref(even))
    teams = [("world", world, list(range(P)))]
    if even.value:
        teams.append(("even", even.value, list(range(0, P, 2))))

    def check(exp, got, what):
        nonlocal checks
        checks += 1
        mm = R.mismatches(exp, got, 1)
        if mm:
            bad.append(what + (mm,))

    def run_all(tag, members, idx, es, n, modes, fcollect, alltoall, alltoalls):
        """The three collectives of one (team, type, size) in every buffer mode."""
        m = len(members)
        B, N = n * es, m * n
        seed = zlib.crc32(f"{tag}/{es}/{n}".encode())
        srcs = [fill(seed, q, B) for q in members]
        exp = np.concatenate(srcs)
        for mode in modes:
            got = bufs.run(mode, srcs[idx], np.full(m * B, SENTINEL, np.uint8), fcollect)
            check(exp, got, (tag, "fcollect", es, n, mode))
        srcs = [fill(seed + 1, q, m * B) for q in members]
        exp = np.concatenate([srcs[j][idx * B:(idx + 1) * B] for j in range(m)])
        for mode in modes:
            got = bufs.run(mode, srcs[idx], np.full(m * B, SENTINEL, np.uint8), alltoall)
            check(exp, got, (tag, "alltoall", es, n, mode))
        for dst, sst in STRIDES:
            src = spread(srcs[idx], N, sst, es)
            init = np.full(extent(N, dst, es), SENTINEL, np.uint8)
            want = spread(exp, N, dst, es)  # the gaps still hold the sentinel
            for mode in modes:
                got = bufs.run(mode, src, init, lambda d, s: alltoalls(d, s, dst, sst))
                check(want, got, (tag, "alltoalls", dst, sst, es, n, mode))

    for tname, team, members in teams:
        if me not in members:
            continue
        idx = members.index(me)
        for ty, es in TYPES.items():
            if ty == "mem":
                fns = (S.shmem_fcollectmem, S.shmem_alltoallmem, S.shmem_alltoallsmem)
            else:
                fns = tuple(getattr(S, f"shmem_{ty}_{k}") for k in ("fcollect", "alltoall", "alltoalls"))
            for n in SIZES + ([BIG] if ty == "int" else []):
                modes = MODES if n <= max(SIZES) else ("heap", "device")
                run_all(f"{tname}/{ty}", members, idx, es, n, modes,
                        lambda d, s: fns[0](team, d, s, n),
                        lambda d, s: fns[1](team, d, s, n),
                        lambda d, s, dst, sst: fns[2](team, d, s, dst, sst, n))
    # ---- the deprecated active-set forms over the world ------------------------------------
    for bits in (32, 64):
        fc, a2a, a2as = (getattr(S, f"shmem_{k}{bits}") for k in ("fcollect", "alltoall", "alltoalls"))
        for n in (1, 37, 5003):
            run_all(f"as{bits}", list(range(P)), me, bits // 8, n, ("heap", "host"),
                    lambda d, s: fc(d, s, n, 0, 0, P, psync),
                    lambda d, s: a2a(d, s, n, 0, 0, P, psync),
                    lambda d, s, dst, sst: a2as(d, s, dst, sst, n, 0, 0, P, psync))
    # zero elements: nothing moves, nothing is written
    init = np.full(64, SENTINEL, np.uint8)
    for mode in ("heap", "host"):
        for call in (lambda d, s: S.shmem_int_fcollect(world, d, s, 0),
                     lambda d, s: S.shmem_int_alltoall(world, d, s, 0),
                     lambda d, s: S.shmem_int_alltoalls(world, d, s, 2, 3, 0)):
            check(init, bufs.run(mode, init, init, call), ("zero", mode))
    # pSync is left at SHMEM_SYNC_VALUE
    ps = np.ctypeslib.as_array((ctypes.c_uint8 * (8 * 64)).from_address(psync))
    check(np.zeros(8 * 64, np.uint8), ps, ("psync",))
    S.shmem_barrier_all()
    S.shmemx_free_device(hdst)
    S.shmemx_free_device(hsrc)
    S.shmem_free(psync)
    S.shmem_free(hh[1])
    S.shmem_free(hh[0])
    if even.value:
        S.lib().shmem_team_destroy(even)
    sig = {1: "stream", 0: "host"}.get(L.lib().sosx_p2p_signal_mode(), "none")
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} checks OK (p2p signal {sig})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
