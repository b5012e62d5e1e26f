#!/usr/bin/env python3
"""Block-strided put against its two yardsticks, on one MI355X.

Run under tools/oshrun with one PE (the self-PE forms) or two PEs sharing the GPU (PE 0
puts into PE 1's heap through the IPC mapping; PE 1 waits at a barrier):

  SHMEMX_TRANSPORT=p2p SHMEMX_DEVICE_HEAP_SIZE=1536M SHMEMX_STAGE_BYTES=64M \\
      python tools/oshrun -np 2 python tools/rma_bench.py

For each block size (64 B, 1 KiB, 64 KiB; 256 MiB moved; both strides twice the block) it
times, alternating the three in every repetition:

  ibput     shmemx_ibput8 (sosx_block_strided_copy + the completing system-scope release)
  memcpy2d  hipMemcpy2DAsync on the same pointers and shape + hipStreamSynchronize
  put       shmem_putmem of the same 256 MiB, contiguous

and once the same ibput shape with the source 4 B off the target's 16-B grid (the
incongruent regime, unaligned 16-B loads).  A timed window is BATCH back-to-back calls,
each ending in a device synchronise, under one host clock (tens of milliseconds: a single
0.1-0.2 ms call is too short a window to resolve a few per cent); the figure is the
window over BATCH: whole-call time, not kernel time.  Warm-up: one window per form; then
WINDOWS windows per form, the forms alternating.  Reported per call: median, min and max
over the windows in ms, the spread (max - min) / median, and the median's rate as payload
GB/s (256 MiB / time; the HBM traffic is twice that: one read and one write).  Two forms
whose [min, max] ranges overlap are not told apart by this run.
"""
import ctypes
import statistics
import sys
import os
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402,F401

from sos_amd import _lib as L  # noqa: E402
from sos_amd import shmem as S  # noqa: E402

TOTAL = 256 << 20
BATCH, WINDOWS = 200, 9


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    pe = 1 if P > 1 else 0
    tgt = S.shmemx_malloc_device(2 * TOTAL + 64)
    src = S.shmemx_malloc_device(2 * TOTAL + 64)
    assert tgt and src, "device heap too small: SHMEMX_DEVICE_HEAP_SIZE=1536M"
    hip = L.lib()
    hip.hipMemcpy2DAsync.restype = ctypes.c_int
    hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.restype = ctypes.c_int
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipMemset(src, 0x5A, 2 * TOTAL + 64)
    hip.hipMemset(tgt, 0, 2 * TOTAL + 64)
    stream = S.lib().shmemx_get_stream()
    remote = S.shmem_ptr(tgt, pe)  # where PE `pe`'s tgt is mapped here (its own address on one PE)
    S.shmem_barrier_all()
    if me == 0:
        print(f"# rma_bench: {P} PE(s), target on PE {pe} ({'self' if pe == me else 'peer, same GPU'}), "
              f"{TOTAL >> 20} MiB per call, windows of {BATCH} calls, {WINDOWS} windows per form, per-call ms")
        print(f"# {'form':<28} {'block':>8} {'median ms':>10} {'min ms':>8} {'max ms':>8} {'spread':>7} {'GB/s':>8}")
        for block in (64, 1 << 10, 64 << 10):
            nblocks = TOTAL // block

            def ibput(soff=0):
                S.shmemx_ibput8(tgt, src + soff, 2 * block, 2 * block, block, nblocks, pe)

            def memcpy2d():
                rc = hip.hipMemcpy2DAsync(remote, 2 * block, src, 2 * block, block, nblocks, 3, stream)
                assert rc == 0, rc
                assert hip.hipStreamSynchronize(stream) == 0

            def put():
                S.shmem_putmem(tgt, src, TOTAL, pe)

            forms = [("ibput (congruent)", ibput), ("hipMemcpy2DAsync", memcpy2d), ("putmem (contiguous)", put),
                     ("ibput (source +4 B)", lambda: ibput(4))]
            times = {name: [] for name, _ in forms}

            def window(fn):
                t0 = time.perf_counter()
                for _ in range(BATCH):
                    fn()
                return (time.perf_counter() - t0) * 1e3 / BATCH

            for name, fn in forms:
                window(fn)
            for _ in range(WINDOWS):
                for name, fn in forms:
                    times[name].append(window(fn))
            for name, _ in forms:
                t = times[name]
                med = statistics.median(t)
                print(f"  {name:<28} {block:>8} {med:>10.4f} {min(t):>8.4f} {max(t):>8.4f} "
                      f"{(max(t) - min(t)) / med:>6.1%} {TOTAL / med / 1e6:>8.1f}", flush=True)
    S.shmem_barrier_all()
    S.shmemx_free_device(src)
    S.shmemx_free_device(tgt)
    S.shmem_finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
