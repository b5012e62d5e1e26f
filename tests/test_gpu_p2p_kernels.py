"""GPU: the device side of the p2p transport at kernel level -- the gated gather
(sosx_gather_signalled: k_gather<true>, or k_p2p_signal before k_gather<false>) and the
signalling step (sosx_p2p_signal: k_p2p_signal, several launches above 64 entries).

Counters and the error word are 64-bit words in pinned host memory, one per 64-B line, as
the transport's are.  Every wait a case issues is already met when it runs -- by the
call's own stores (each wait on a store that another lane or a later store launch makes, so
the stores must all come first), or by a value the host wrote before the call -- so no case
waits on anything; the limit (one second of the device's wall clock,
converted by the library as the transport converts its own) only turns a wrong order into
a failed assertion rather than a hang.  Expiry itself stays with the multi-PE timeout
tests.
"""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from sos_amd import _lib

pytestmark = pytest.mark.gpu

LINE = 8           # 64-bit words per 64-B line
NWORDS = 320       # counters a case may touch: stored ones from 0, host-set ones from PRESET
PRESET = 160
TILE = 256 * 4 * 16  # bytes of one tile (gather_plan.h kTileVec vectors of 16 B)
NONE, FUSED, BEFORE, ALONE = 0, 1, 2, 3
LIMIT_S = 1.0


class Words:
    """NWORDS counters and the error word, each on a 64-B line of its own."""

    def __init__(self, torch):
        self.t = torch.zeros((NWORDS + 1) * LINE, dtype=torch.int64, pin_memory=True)
        self.base = self.t.data_ptr()
        assert self.base % 64 == 0

    def addr(self, k):
        return self.base + 64 * k

    @property
    def err_addr(self):
        return self.addr(NWORDS)

    def view(self):
        return self.t.view(-1, LINE)[:, 0].numpy()  # the words themselves (shares the memory)

    def clear(self):
        self.t.zero_()


@pytest.fixture(scope="module")
def words(torch_cuda):
    return Words(torch_cuda)


@pytest.fixture(scope="module")
def limit(torch_cuda):
    ticks = _lib.lib().sosx_p2p_ticks(torch_cuda.cuda.current_device(), LIMIT_S)
    assert ticks > 0, "the device reports no wall-clock rate"
    return ticks


def step_args(words, nw, nq, call):
    """nw stores and nq waits.  Wait i < nw awaits stored word nw - 1 - i at its stored
    value: the first waits await the LAST stores, which another lane makes and, above 64
    stores, a later store launch -- a wait issued before every store has been would expire.
    The other waits await words the host sets here, every third of them already above the
    wanted value (>=).  Returns the ctypes arguments and the expected words afterwards."""
    w = words.view()
    wa = [words.addr(i) for i in range(nw)]
    wv = [call * 1000 + i + 1 for i in range(nw)]
    qa, qv = [], []
    expect = np.zeros(NWORDS + 1, np.int64)
    expect[:nw] = wv
    for i in range(nq):
        if i < nw:
            qa.append(wa[nw - 1 - i])
            qv.append(wv[nw - 1 - i])
        else:
            want = call * 77 + i + 1
            w[PRESET + i] = want + (5 if i % 3 == 0 else 0)
            expect[PRESET + i] = w[PRESET + i]
            qa.append(words.addr(PRESET + i))
            qv.append(want)

    def arr(ty, xs):
        return (ty * len(xs))(*xs) if xs else None
    return (nw, arr(ctypes.c_void_p, wa), arr(ctypes.c_uint64, wv), nq, arr(ctypes.c_void_p, qa),
            arr(ctypes.c_uint64, qv)), expect


# ------------------------------------------------------------------------------------
# sosx_gather_signalled
# ------------------------------------------------------------------------------------
GATHER_CASES = {
    # name: (segments (src offset, dst offset, bytes), nw, nq, the gate placement)
    "fused": ([(1, 2, 1), (5, 0, 40000), (0, 7, 12345)], 3, 3, FUSED),
    "own_step_tiles": ([(3, 3, 17 * TILE + 5)], 2, 2, BEFORE),
    "own_step_count": ([(i % 16, (3 * i) % 16, 100 + 37 * i) for i in range(17)], 2, 3, BEFORE),
    "twenty_four_empty": ([(i % 16, (5 * i) % 16, 0 if i < 4 else 1000 + 61 * i) for i in range(20)],
                          3, 3, FUSED),
    "nothing_copied": ([(0, 0, 0), (3, 5, 0), (9, 1, 0)], 2, 2, ALONE),
    "no_stores_no_waits": ([(1, 2, 1), (4, 0, 40000), (0, 7, 33)], 0, 0, FUSED),
    "sixteen_each": ([(2, 9, 31), (8, 0, 40000), (0, 0, 16)], 16, 16, FUSED),
    "waits_only": ([(6, 6, 17), (0, 12, 20000)], 0, 16, FUSED),
    "stores_only": ([(15, 1, 15), (12, 0, 20000)], 16, 0, FUSED),
}
COPYING = [k for k in GATHER_CASES if k != "nothing_copied"]


def make_segments(torch, segs, rng):
    srcs, dsts = [], []
    for so, do, n in segs:
        s = torch.from_numpy(rng.integers(0, 256, n + 64, dtype=np.uint8)).cuda()
        d = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        srcs.append(s)
        dsts.append(d)
    return srcs, dsts


def seg_args(segs, srcs, dsts):
    k = len(segs)
    sp = [s.data_ptr() + so for s, (so, _, _) in zip(srcs, segs)]
    dp = [d.data_ptr() + do for d, (_, do, _) in zip(dsts, segs)]
    nb = [n for _, _, n in segs]
    return sp, dp, nb, (k, (ctypes.c_void_p * k)(*sp), (ctypes.c_void_p * k)(*dp), (ctypes.c_size_t * k)(*nb))


@pytest.mark.parametrize("case", list(GATHER_CASES))
def test_gather_signalled(torch_cuda, words, limit, case):
    """Every destination byte equals its source byte and the 0xA5 guards around every
    destination stay; every stored word holds its value, the words beyond are untouched and
    *err stays 0 -- whether the step rides in the copy launch, runs before it, or alone."""
    torch = torch_cuda
    segs, nw, nq, gate = GATHER_CASES[case]
    rng = np.random.default_rng(len(case) * 1009 + nw)
    srcs, dsts = make_segments(torch, segs, rng)
    sp, dp, nb, sargs = seg_args(segs, srcs, dsts)
    assert _lib.gather_plan(sp, dp, nb, gated=True)["gate"] == gate  # the path the case is named for
    words.clear()
    gargs, expect = step_args(words, nw, nq, 3)
    torch.cuda.synchronize()
    rc = _lib.lib().sosx_gather_signalled(*sargs, *gargs, words.err_addr, limit, None)
    assert rc == 0
    torch.cuda.synchronize()
    for (so, do, n), s, d in zip(segs, srcs, dsts):
        assert torch.equal(d[do:do + n], s[so:so + n]), (case, so, do, n)
        assert bool((d[:do] == 0xA5).all()) and bool((d[do + n:] == 0xA5).all()), (case, so, do, n)
    assert np.array_equal(words.view(), expect), case  # stored values, nothing beyond, *err == 0


def test_gather_signalled_refuses(torch_cuda, words, limit):
    """17 stores, 17 waits, or waits without an error word: SOSX_ERR_ARG, nothing changed."""
    torch = torch_cuda
    segs = [(1, 2, 5000)]
    srcs, dsts = make_segments(torch, segs, np.random.default_rng(5))
    _, _, _, sargs = seg_args(segs, srcs, dsts)
    words.clear()
    f = _lib.lib().sosx_gather_signalled
    wa = (ctypes.c_void_p * 17)(*[words.addr(i) for i in range(17)])
    wv = (ctypes.c_uint64 * 17)(*range(1, 18))
    zero = (ctypes.c_uint64 * 17)()
    torch.cuda.synchronize()
    assert f(*sargs, 17, wa, wv, 0, None, None, words.err_addr, limit, None) == -3
    assert f(*sargs, 0, None, None, 17, wa, zero, words.err_addr, limit, None) == -3
    assert f(*sargs, 1, wa, wv, 1, wa, zero, None, limit, None) == -3
    assert f(*sargs, -1, wa, wv, 0, None, None, words.err_addr, limit, None) == -3
    torch.cuda.synchronize()
    assert bool((dsts[0] == 0xA5).all())
    assert not words.view().any()


def test_gather_signalled_dpp_shape_forced():
    """SOSX_GATHER_REALIGN=0 (every incongruent source by the DPP shape): the copying cases
    above rerun in a child process."""
    here = os.path.abspath(__file__)
    # by node id: a case added later cannot drop out of the child by its name
    ids = [f"{here}::test_gather_signalled[{c}]" for c in COPYING]
    r = subprocess.run([sys.executable, "-m", "pytest", *ids, "-q", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=200,
                       env=dict(os.environ, SOSX_GATHER_REALIGN="0"), cwd=os.path.dirname(os.path.dirname(here)))
    assert r.returncode == 0, (r.stdout[-2500:], r.stderr[-1500:])
    assert f"{len(COPYING)} passed" in r.stdout


# ------------------------------------------------------------------------------------
# sosx_p2p_signal
# ------------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 150]


@pytest.mark.parametrize("nq", COUNTS)
@pytest.mark.parametrize("nw", COUNTS)
def test_p2p_signal(torch_cuda, words, limit, nw, nq):
    """Up to 150 stores and 150 waits: 64 per launch, every store launch before the first
    wait launch.  The waits are on the stored words in reverse order as far as those
    reach: wait 0 awaits the last store, so with more than 64 stores a wait issued along
    with the first store launch awaits a word of a later one, runs into the limit and
    sets *err."""
    torch = torch_cuda
    words.clear()
    args, expect = step_args(words, nw, nq, 5)
    torch.cuda.synchronize()
    rc = _lib.lib().sosx_p2p_signal(*args, words.err_addr, limit, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = words.view()
    assert got[NWORDS] == 0, "a wait expired: it ran before the store it awaits"
    assert np.array_equal(got, expect), (nw, nq)  # nw = nq = 0: nothing at all


def test_p2p_signal_refuses(torch_cuda, words, limit):
    words.clear()
    f = _lib.lib().sosx_p2p_signal
    wa = (ctypes.c_void_p * 1)(words.addr(0))
    one = (ctypes.c_uint64 * 1)(1)
    assert f(-1, wa, one, 0, None, None, words.err_addr, limit, None) == -3
    assert f(0, None, None, -1, wa, one, words.err_addr, limit, None) == -3
    assert f(0, None, None, 1, wa, one, None, limit, None) == -3  # waits need the error word
    torch_cuda.cuda.synchronize()
    assert not words.view().any()


def test_p2p_signal_gives_up_after_an_earlier_timeout(torch_cuda, words, limit):
    """*err already set (an earlier step of the call expired): a step's waits return at
    once.  The one wait here is not met; with the error word honoured the call and its
    synchronisation end far inside the limit -- half of it is the condition, derived from
    the limit the call was given."""
    torch = torch_cuda
    f = _lib.lib().sosx_p2p_signal
    words.clear()
    wa = (ctypes.c_void_p * 1)(words.addr(1))
    one = (ctypes.c_uint64 * 1)(1)
    assert f(1, wa, one, 0, None, None, None, limit, None) == 0  # the kernel is loaded
    torch.cuda.synchronize()
    w = words.view()
    assert w[1] == 1
    w[NWORDS] = 1
    qa = (ctypes.c_void_p * 1)(words.addr(0))
    five = (ctypes.c_uint64 * 1)(5)
    t0 = time.perf_counter()
    assert f(0, None, None, 1, qa, five, words.err_addr, limit, None) == 0
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    assert elapsed < LIMIT_S / 2, f"the step waited {elapsed:.3f} s with *err set"
    assert w[NWORDS] == 1 and w[0] == 0
