"""Multi-PE correctness run of the distributed locks (one process per PE, tools/oshrun, p2p
transport): shmem_set_lock, shmem_clear_lock and shmem_test_lock guarding a counter and a log
on PE 0's device heap.

  * K rounds per PE of set_lock, g the counter, p own id into log[counter], p counter + 1,
    clear_lock: a lost update, or a put of the critical section not complete before the lock
    moved on, shows as a wrong final counter or a log slot written twice or never;
  * 10 more rounds per PE that take the lock through a shmem_test_lock polling loop bounded
    by an iteration count;
  * after a barrier: counter = P * (K + 10), every log slot written and every PE there
    K + 10 times, the lock word zero on every PE;
  * shmem_test_lock returns 0 on a free lock and 1 while another PE is known to hold it (the
    holder keeps it across a barrier pair).

SHMEMX_P2P_TIMEOUT bounds every wait: a lost hand-off ends the job with a message.  Prints one
line per PE, exit 0 = OK.
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

K = 25
TRIES = 10
POLL_LIMIT = 200000


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    bad, checks = [], 0
    total = P * (K + TRIES)

    def expect(want, got, what):
        nonlocal checks
        checks += 1
        if want != got:
            bad.append((what, "want", want, "got", got))

    # [lock | counter | log[total]] at the same offset on every PE; PE 0's copy is the shared one
    nbytes = 8 * (2 + total)
    buf = S.shmemx_malloc_device(nbytes)
    assert buf
    lock, counter, log = buf, buf + 8, buf + 16
    init = np.full(2 + total, -1, np.int64)
    init[0] = init[1] = 0
    S.shmem_putmem(buf, init.ctypes.data, nbytes, me)
    S.shmem_quiet()
    S.shmem_barrier_all()

    def critical_section(what):
        c = S.shmem_long_g(counter, 0)
        expect(True, 0 <= c < total, (what, "counter in range", c))
        if 0 <= c < total:
            S.shmem_long_p(log + 8 * c, me, 0)
        S.shmem_long_p(counter, c + 1, 0)

    for k in range(K):
        S.shmem_set_lock(lock)
        critical_section(("set_lock round", k))
        S.shmem_clear_lock(lock)

    for k in range(TRIES):
        for _ in range(POLL_LIMIT):
            if S.shmem_test_lock(lock) == 0:
                critical_section(("test_lock round", k))
                S.shmem_clear_lock(lock)
                break
        else:
            bad.append(("test_lock never got the lock", k))
    S.shmem_barrier_all()

    # ---- the outcome ------------------------------------------------------------------------------------------
    expect(total, S.shmem_long_g(counter, 0), "final counter")
    got = np.empty(total, np.int64)
    S.shmem_getmem(got.ctypes.data, log, 8 * total, 0)
    expect(0, int(np.count_nonzero((got < 0) | (got >= P))), "log slots never written")
    for q in range(P):
        expect(K + TRIES, int(np.count_nonzero(got == q)), ("log entries of PE", q))
    expect(0, int(R.device_bytes(lock, 8).view(np.int64)[0]), "this PE's lock word after the last clear_lock")
    S.shmem_barrier_all()

    # ---- test_lock on a free and on a held lock ---------------------------------------------------------------
    for holder in range(P):
        if me == holder:
            expect(0, S.shmem_test_lock(lock), ("test_lock on a free lock", holder))
            if P == 1:
                expect(1, S.shmem_test_lock(lock), "test_lock on the lock this PE holds")
        S.shmem_barrier_all()
        if me != holder:
            expect(1, S.shmem_test_lock(lock), ("test_lock while another PE holds the lock", holder))
        S.shmem_barrier_all()
        if me == holder:
            S.shmem_clear_lock(lock)
        S.shmem_barrier_all()
    expect(0, int(R.device_bytes(lock, 8).view(np.int64)[0]), "this PE's lock word at the end")

    steps, probes = ctypes.c_long(), ctypes.c_long()
    S.sosx_lock_stats(ctypes.byref(steps), ctypes.byref(probes))
    a_, r_, u_ = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    L.lib().sosx_acquire_stats(ctypes.byref(a_), ctypes.byref(r_), ctypes.byref(u_), None)
    if u_.value:
        bad.append(("unacquired peer reads", u_.value))
    S.shmem_barrier_all()
    S.shmemx_free_device(buf)
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} checks OK (lock launches {steps.value}, probes {probes.value}, "
          f"{u_.value} unacquired)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
