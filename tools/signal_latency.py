"""Per-call time of put-with-signal, fused against composed, and the hand-off latency of
put_signal + signal_wait_until against put + quiet + barrier.

    SHMEMX_TRANSPORT=p2p tools/oshrun -np 2 python tools/signal_latency.py [--reps 5]

2 PEs on ONE GPU, every PE sending to (me + 1) % P, both sides in the device heap.

Table 1, the fused limit: microseconds per call from the host wall clock around windows of
back-to-back calls, each window ended by one shmem_quiet; median and spread (max - min) over
the repetitions, the two forms alternating, max over PEs.
  A  shmem_putmem_signal_nbi through the fused kernel (limit raised above every size)
  B  shmem_putmem_nbi + shmem_fence + shmem_uint64_atomic_set: what the library offered before
Sizes 8 B .. 32 MiB in powers of 4, and 64 MiB.  The default of SHMEMX_PUT_SIGNAL_FUSED_MAX is
the largest size up to which A's median is below B's by more than the larger spread.

Table 2, the hand-off: a ping-pong between PE 0 and PE 1 at 8 B and 64 KiB, microseconds per
one-way hand-off (round trip / 2):
  signal (fused) / signal (composed)  put_signal_nbi + signal_wait_until(GE, round)
  barrier                             put + quiet + shmem_barrier_all on both PEs
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sos_amd import shmem as S  # noqa: E402

SIZES = [8 * 4 ** k for k in range(12)] + [64 << 20]
SET, GE = 0, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=200)
    a = ap.parse_args()
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    peer = (me + 1) % P
    nmax = max(SIZES)
    target, source, sig = S.shmemx_malloc_device(nmax), S.shmemx_malloc_device(nmax), S.shmemx_malloc_device(64)
    nrow = len(SIZES) * 4 + 16
    stats, out = S.shmem_malloc(8 * nrow), S.shmem_malloc(8 * nrow)
    res = (ctypes.c_double * nrow).from_address(stats)
    S.shmemx_signal_set(sig, 0, me)
    S.shmem_barrier_all()
    default_limit = S.sosx_set_put_signal_fused_max(1 << 40)

    def form_a(n, calls):
        for _ in range(calls):
            S.shmem_putmem_signal_nbi(target, source, n, sig, 1, SET, peer)
        S.shmem_quiet()

    def form_b(n, calls):
        for _ in range(calls):
            S.shmem_putmem_nbi(target, source, n, peer)
            S.shmem_fence()
            S.shmem_uint64_atomic_set(sig, 1, peer)
        S.shmem_quiet()

    for i, n in enumerate(SIZES):
        calls = max(2, min(32, (256 << 20) // n))
        form_a(n, 2)
        form_b(n, 2)
        S.shmem_barrier_all()
        us = {"A": [], "B": []}
        for _ in range(a.reps):
            for key, form in (("A", form_a), ("B", form_b)):
                t0 = time.perf_counter()
                form(n, calls)
                us[key].append((time.perf_counter() - t0) * 1e6 / calls)
                S.shmem_barrier_all()
        for j, key in enumerate(("A", "B")):
            res[4 * i + 2 * j], res[4 * i + 2 * j + 1] = statistics.median(us[key]), max(us[key]) - min(us[key])

    # ---- hand-off: PE 0 <-> PE 1 --------------------------------------------------------------------------------
    base = 4 * len(SIZES)
    rows = []
    if P >= 2:
        other = 1 - me if me < 2 else me

        def pingpong_signal(n, rounds, r0):
            for r in range(r0 + 1, r0 + rounds + 1):
                if me == 0:
                    S.shmem_putmem_signal_nbi(target, source, n, sig + 8, r, SET, other)
                    S.shmem_signal_wait_until(sig + 8, GE, r)
                elif me == 1:
                    S.shmem_signal_wait_until(sig + 8, GE, r)
                    S.shmem_putmem_signal_nbi(target, source, n, sig + 8, r, SET, other)
            S.shmem_quiet()

        def pingpong_barrier(n, rounds, r0):
            for _ in range(rounds):
                if me == 0:
                    S.shmem_putmem(target, source, n, other)
                    S.shmem_quiet()
                S.shmem_barrier_all()
                if me == 1:
                    S.shmem_putmem(target, source, n, other)
                    S.shmem_quiet()
                S.shmem_barrier_all()

        S.shmemx_signal_set(sig + 8, 0, me)
        S.shmem_barrier_all()
        seen = 0
        k = 0
        for n in (8, 64 << 10):
            for name, limit, fn in (("signal (fused)", 1 << 40, pingpong_signal), ("signal (composed)", 0, pingpong_signal),
                                    ("barrier", 0, pingpong_barrier)):
                S.sosx_set_put_signal_fused_max(limit)
                fn(n, 20, seen)
                seen += 20 if fn is pingpong_signal else 0
                S.shmem_barrier_all()
                us = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn(n, a.rounds, seen)
                    us.append((time.perf_counter() - t0) * 1e6 / (2 * a.rounds))
                    seen += a.rounds if fn is pingpong_signal else 0
                    S.shmem_barrier_all()
                res[base + 2 * k], res[base + 2 * k + 1] = statistics.median(us), max(us) - min(us)
                rows.append((n, name))
                k += 1
    S.sosx_set_put_signal_fused_max(default_limit)
    S.shmem_double_max_reduce(S.team_world(), out, stats, nrow)
    tot = (ctypes.c_double * nrow).from_address(out)
    if me == 0:
        print(f"# {P} PEs on one GPU, target on PE (me + 1) % P; {a.reps} repetitions; us per call, median (spread), max over PEs")
        print(f"# default SHMEMX_PUT_SIGNAL_FUSED_MAX of this build: {default_limit}")
        print("# table 1: A fused put_signal_nbi, B putmem_nbi + fence + uint64_atomic_set; windows ended by quiet")
        limit = 0
        still = True
        for i, n in enumerate(SIZES):
            am, asp, bm, bsp = tot[4 * i:4 * i + 4]
            wins = am < bm - max(asp, bsp)
            still = still and wins
            if still:
                limit = n
            print(f"P={P} bytes={n:9d}: A {am:9.2f} ({asp:7.2f})   B {bm:9.2f} ({bsp:7.2f})   {'A' if wins else '-'}")
        print(f"# largest size up to which A wins by more than the spread: {limit}")
        if rows:
            print(f"# table 2: one-way hand-off between PE 0 and PE 1, {a.rounds} round trips per repetition")
            for k, (n, name) in enumerate(rows):
                print(f"P={P} bytes={n:6d} {name:18s}: {tot[base + 2 * k]:8.2f} us (spread {tot[base + 2 * k + 1]:.2f})")
        sys.stdout.flush()
    S.shmem_barrier_all()
    for p in (out, stats):
        S.shmem_free(p)
    for p in (sig, source, target):
        S.shmemx_free_device(p)
    S.shmem_finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
