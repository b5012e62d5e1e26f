"""Multi-PE correctness run of shmem_collect (one process per PE).

Run under tools/oshrun: every PE calls shmem_<T>_collect, shmem_collectmem (over
SHMEM_TEAM_WORLD and an even-PE split team) and the deprecated shmem_collect32/64 (over
the world) with per-PE element counts that differ between PEs -- ragged, zero on some
PEs, zero on all, one long contribution among short ones, all equal -- on device-heap
buffers (shmemx_malloc_device), plain device buffers, pageable host buffers and host
symmetric-heap buffers.  Every member's input is regenerated on the CPU from a seed and
the PE's own target is compared with the plain concatenation

  target = concat over members q of source(q)          (src/collectives.c:1215-1276)

and the bytes of the target above the concatenation with the sentinel they held before.
Small reductions and broadcasts on the same team run between the collect calls and are
checked too.  At the end the library's own count of peer reads that followed a wait
without an acquire (sosx_acquire_stats) must be 0, and pSync must hold SHMEM_SYNC_VALUE.

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
from tests.collect_check_pe import Buffers  # noqa: E402

TYPES = {"int": 4, "double": 8, "uint8": 1, "longdouble": 16, "mem": 1}
MODES = ("heap", "device", "host", "hostheap")
SENTINEL = 0x6B
TAIL = 64
BIG = (1 << 18) + 3   # elements of the long contribution (int only): above every payload cap


def small_expected(P, lens, mode):
    """Does this call take the one-kernel small path?  Mirrors smallpath.cpp collect_cap with
    the default SHMEMX_SMALL_HOST_BYTES (1 MiB slots) and SHMEMX_SMALL_DEVICE (128 KiB):
    every member's length must be at most the cap of its source's residency."""
    if P < 2 or os.environ.get("SHMEMX_SMALL_COLLECT") == "0":
        return False
    slot = 1 << 20
    cap = min(slot - 16, slot // P, 64 << 10)
    if mode in ("heap", "device"):
        cap = min(cap, (128 << 10) // P, 16 << 10)
    # a zero length has no residency: it always fits
    return all(n <= cap for n in lens)


def vectors(m):
    """name -> element counts per member index."""
    return {"ragged": [i + 1 for i in range(m)],
            "some_zero": [37 if i % 2 else 0 for i in range(m)],
            "all_zero": [0] * m,
            "first_only": [255] + [0] * (m - 1),
            "equal": [5003] * m}


def acquire_stats():
    a, r, u = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    L.lib().sosx_acquire_stats(ctypes.byref(a), ctypes.byref(r), ctypes.byref(u), None)
    return a.value, r.value, u.value


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    world = S.team_world()
    bad, checks = [], 0
    stats = {"small": 0, "executor": 0}
    heap_bytes = 4 * (BIG + 3 * P) + 16 * 5003 * P + TAIL
    hsrc = S.shmemx_malloc_device(heap_bytes)
    hdst = S.shmemx_malloc_device(heap_bytes)
    hh = (S.shmem_malloc(heap_bytes), S.shmem_malloc(heap_bytes))
    psync = S.shmem_malloc(8 * 64)
    ctypes.memset(psync, 0, 8 * 64)
    # operands of the interleaved small calls: host symmetric heap, 8 ints
    sm_in, sm_out = S.shmem_malloc(64), S.shmem_malloc(64)
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

    def small_calls(team, members, idx, k):
        """A small reduction and a small broadcast on `team` between two collect calls."""
        m = len(members)
        a = np.ctypeslib.as_array((ctypes.c_int32 * 8).from_address(sm_in))
        out = np.ctypeslib.as_array((ctypes.c_int32 * 8).from_address(sm_out))
        a[:] = np.arange(8, dtype=np.int32) + 10 * idx + k
        out[:] = -1
        S.shmem_int_sum_reduce(team, sm_out, sm_in, 8)
        want = sum(np.arange(8, dtype=np.int64) + 10 * i + k for i in range(m)).astype(np.int32)
        check(want.view(np.uint8), out.copy().view(np.uint8), ("reduce", k))
        if m == 1:
            # a team broadcast in a one-PE job aborts under the p2p transport (p2p_exec has
            # no shared segment to run on; INTEGRATION.md "Known gaps"): not this file's subject
            return
        root = k % m
        out[:] = -1
        S.shmem_int_broadcast(team, sm_out, sm_in, 8, root)
        want = (np.arange(8, dtype=np.int32) + 10 * root + k)
        check(want.view(np.uint8), out.copy().view(np.uint8), ("broadcast", k))

    def run(tag, members, idx, es, counts, modes, call):
        lens = [n * es for n in counts]
        total = sum(lens)
        seed = zlib.crc32(f"{tag}/{es}/{counts[:4]}".encode())
        srcs = [np.random.default_rng(seed + q).integers(0, 256, lens[i], dtype=np.uint8)
                for i, q in enumerate(members)]
        exp = np.concatenate(srcs + [np.full(TAIL, SENTINEL, np.uint8)])
        for mode in modes:
            src = srcs[idx] if lens[idx] else np.full(16, 0x11, np.uint8)  # a place, not read
            before = L.lib().sosx_small_collect_calls()
            want_small = small_expected(len(members), lens, mode)
            got = bufs.run(mode, src, np.full(total + TAIL, SENTINEL, np.uint8),
                           lambda d, s: call(d, s, counts[idx]))
            check(exp, got, (tag, es, tuple(counts[:4]), mode))
            took = L.lib().sosx_small_collect_calls() - before
            stats["small" if took else "executor"] += 1
            if took != (1 if want_small else 0):
                bad.append((tag, mode, "small path taken" if took else "small path not taken"))

    k = 0
    for tname, team, members in teams:
        if me not in members:
            continue
        idx, m = members.index(me), len(members)
        for ty, es in TYPES.items():
            fn = S.shmem_collectmem if ty == "mem" else getattr(S, f"shmem_{ty}_collect")
            vs = vectors(m)
            if ty == "int":
                vs["long_among_short"] = [BIG if i == m // 2 else 1 + i % 3 for i in range(m)]
            for name, counts in vs.items():
                modes = MODES if ty in ("int", "mem") else ("heap", "host")
                run(f"{tname}/{ty}/{name}", members, idx, es, counts, modes,
                    lambda d, s, n: fn(team, d, s, n))
                small_calls(team, members, idx, k)
                k += 1
    # ---- the deprecated active-set forms over the world ------------------------------------
    for bits in (32, 64):
        fc = getattr(S, f"shmem_collect{bits}")
        for name, counts in vectors(P).items():
            run(f"as{bits}/{name}", list(range(P)), me, bits // 8, counts, ("heap", "host"),
                lambda d, s, n: fc(d, s, n, 0, 0, P, psync))
    if P >= 2:  # a strided active set: the even PEs
        m = (P + 1) // 2
        if me % 2 == 0:
            run("as32/even", list(range(0, P, 2)), me // 2, 4, [3 * i + 1 for i in range(m)], ("heap",),
                lambda d, s, n: S.shmem_collect32(d, s, n, 0, 1, m, psync))
    # pSync is left at SHMEM_SYNC_VALUE
    ps = np.ctypeslib.as_array((ctypes.c_uint8 * (8 * 64)).from_address(psync))
    check(np.zeros(8 * 64, np.uint8), ps, ("psync",))
    acq, reads, unacq = acquire_stats()
    if unacq:
        bad.append(("unacquired peer reads", unacq))
    S.shmem_barrier_all()
    for p in (sm_out, sm_in, psync, hh[1], hh[0]):
        S.shmem_free(p)
    S.shmemx_free_device(hdst)
    S.shmemx_free_device(hsrc)
    if even.value:
        S.lib().shmem_team_destroy(even)
    sig = {1: "stream", 0: "host"}.get(L.lib().sosx_p2p_signal_mode(), "none")
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} checks OK (p2p signal {sig}, {reads} peer reads, "
          f"{unacq} unacquired, {stats['small']} small, {stats['executor']} executor)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
