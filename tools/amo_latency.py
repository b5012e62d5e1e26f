"""Per-call time of the atomic memory operations, next to a one-element get and put.

    tools/oshrun -np 2 python tools/amo_latency.py [--calls 200] [--reps 5]

2 PEs on ONE GPU (SHMEMX_TRANSPORT=p2p), every operation on a word of the other PE's device
heap.  Rows, microseconds per call, median and spread over the repetitions, max over PEs:

  fetch_add   blocking shmem_long_atomic_fetch_add: one launch and one completion per call
  add burst   256 shmem_long_atomic_add calls ended by ONE shmem_quiet, time per call
  g           shmem_long_g: one copy and one completion per call (the floor to compare with)
  p           shmem_long_p

Wall-clock time on the host around each batch (the calls are synchronous, or ended by the
quiet inside the timed span); one untimed batch first.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sos_amd import shmem as S  # noqa: E402

BURST = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    peer = (me + 1) % P
    word = S.shmemx_malloc_device(64)
    stats = S.shmem_malloc(8 * 8)      # this PE's medians, then everyone's maxima
    out = S.shmem_malloc(8 * 8)
    S.shmem_long_p(word, 0, me)
    S.shmem_barrier_all()
    fadd, add, g, p = S.shmem_long_atomic_fetch_add, S.shmem_long_atomic_add, S.shmem_long_g, S.shmem_long_p

    def burst():
        for _ in range(BURST):
            add(word + 8, 1, peer)
        S.shmem_quiet()

    rows = [("fetch_add", lambda: fadd(word, 1, peer), a.calls, 1),
            ("add burst", burst, max(a.calls // BURST, 4), BURST),
            ("g", lambda: g(word + 16, peer), a.calls, 1),
            ("p", lambda: p(word + 24, 7, peer), a.calls, 1)]
    res = (ctypes.c_double * 8).from_address(stats)
    lines = []
    for i, (name, call, n, per) in enumerate(rows):
        for _ in range(max(n // 4, 1)):   # untimed
            call()
        S.shmem_barrier_all()
        us = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            us.append((time.perf_counter() - t0) * 1e6 / (n * per))
            S.shmem_barrier_all()
        res[2 * i], res[2 * i + 1] = statistics.median(us), max(us) - min(us)
        lines.append((name, n * per))
    S.shmem_double_max_reduce(S.team_world(), out, stats, 8)
    tot = (ctypes.c_double * 8).from_address(out)
    if me == 0:
        print(f"# {P} PEs on one GPU, target word on PE (me + 1) % P; {a.reps} repetitions; us per call, median (spread), "
              f"max over PEs")
        for i, (name, n) in enumerate(lines):
            print(f"P={P} {name:10s} calls/rep={n:5d}: {tot[2 * i]:8.2f} us/call (spread {tot[2 * i + 1]:.2f})")
        sys.stdout.flush()
    S.shmem_barrier_all()
    S.shmem_free(out)
    S.shmem_free(stats)
    S.shmemx_free_device(word)
    S.shmem_finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
