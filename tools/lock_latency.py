"""Time of an uncontended shmem_set_lock + shmem_clear_lock pair, next to the same pair composed
from the public blocking atomics in SOS's sequence.

    tools/oshrun -np 1 python tools/lock_latency.py [--pairs 200] [--reps 7] [--out FILE]
    tools/oshrun -np 2 python tools/lock_latency.py

All PEs on ONE GPU (SHMEMX_TRANSPORT=p2p).  The LAST PE measures and the others wait at a
barrier, so at 2 PEs the home of `last` (PE 0) is remote to the measuring PE.  Rows,
microseconds per pair, median and spread (max - min) over the repetitions:

  fused     shmem_set_lock + shmem_clear_lock: one launch and one completion each (lock.hip)
  composed  SOS's sequence (src/shmem_lock.h) from the public calls on a second lock word:
            shmem_int_atomic_set(data, 0, me), shmem_quiet, shmem_int_atomic_swap(last, me + 1, 0),
            then shmem_quiet, shmem_int_atomic_compare_swap(last, me + 1, 0, 0)

Wall-clock time on the host around each batch of pairs made through ctypes (so each figure
includes the Python calls: two for the fused pair, five for the composed one); one untimed
batch first; the two rows' batches alternate within every repetition.  Appends to --out
(default profiles/lock_latency.txt).  A tool, not a test: nothing in the library depends on
the result.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sos_amd import shmem as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lock_latency.txt"))
    a = ap.parse_args()
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    words = S.shmemx_malloc_device(64)
    S.shmem_putmem(words, bytes(64), 64, me)
    S.shmem_quiet()
    S.shmem_barrier_all()
    lock, last, data = words, words + 32, words + 36   # the composed pair's lock word is a second one
    set_lock, clear_lock, quiet = S.shmem_set_lock, S.shmem_clear_lock, S.shmem_quiet
    aset, swap, cswap = S.shmem_int_atomic_set, S.shmem_int_atomic_swap, S.shmem_int_atomic_compare_swap
    failures = []

    def fused():
        set_lock(lock)
        clear_lock(lock)

    def composed():
        aset(data, 0, me)
        quiet()
        if swap(last, me + 1, 0) != 0:
            failures.append("swap")
        quiet()
        if cswap(last, me + 1, 0, 0) != me + 1:
            failures.append("cswap")

    rows = (("fused", fused), ("composed", composed))
    if me == P - 1:
        for _, call in rows:   # untimed
            for _ in range(max(a.pairs // 4, 8)):
                call()
        us = {name: [] for name, _ in rows}
        for _ in range(a.reps):
            for name, call in rows:
                t0 = time.perf_counter()
                for _ in range(a.pairs):
                    call()
                us[name].append((time.perf_counter() - t0) * 1e6 / a.pairs)
        lines = [f"# {P} PE(s) on one GPU, PE {me} measures, `last` on PE 0; {a.reps} repetitions of {a.pairs} pairs; "
                 f"us per set+clear pair, median (spread = max - min)"]
        for name, _ in rows:
            lines.append(f"P={P} {name:9s}: {statistics.median(us[name]):8.2f} us/pair (spread {max(us[name]) - min(us[name]):.2f})"
                         f"  reps: {' '.join(f'{v:.2f}' for v in us[name])}")
        if failures:
            lines.append(f"# FAILED: the composed sequence met a held lock ({len(failures)} times)")
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        sys.stdout.flush()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    S.shmem_barrier_all()
    S.shmemx_free_device(words)
    S.shmem_finalize()
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
