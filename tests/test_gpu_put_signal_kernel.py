"""GPU: sosx_put_signal (putsignal.hip) in one process, against numpy byte for byte.  The
target is canary-filled with 64 B of slack on both sides and the WHOLE region is compared;
after every launch the signal word holds the expected value (SET: the value; ADD: the
running sum over the sweep) and the ticket word reads 0.  Sizes around the 16-B vector and
the tile, the three sizes at which the grid changes (read from sosx_put_signal_plan), all
16 x 16 source / target residues mod 16 at one small size and four pairs at the others,
both sig_ops.  Bad arguments return SOSX_ERR_ARG without a launch."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64
SET, ADD = 0, 1
ERR_ARG = -3
PAIRS = [(0, 0), (5, 5), (4, 12), (3, 8)]   # congruent aligned / ragged, unaligned loads, single bytes
FIXED = [0, 1, 8, 15, 16, 17, 4095, 4096, 4097]


def plan(S, dst, src, n):
    out = (ctypes.c_longlong * 8)()
    assert S.lib().sosx_put_signal_plan(dst, src, n, out) == 0
    return tuple(out)


def grid_sizes(S):
    """The largest size that still uses one workgroup, that size + 1, and the smallest that
    uses the full grid, for operands on a 16-B boundary: found on the plan function."""
    a, b = 1 << 30, 1 << 31
    full = plan(S, a, b, 1)[7]

    def first(pred):   # smallest n with pred(grid(n)); the grid never shrinks as n grows
        lo, hi = 0, 1 << 30
        while lo + 1 < hi:
            mid = (lo + hi) // 2
            if pred(plan(S, a, b, mid)[6]):
                hi = mid
            else:
                lo = mid
        return hi
    two = first(lambda g: g > 1)
    return two - 1, two, first(lambda g: g >= full)


@pytest.fixture(scope="module")
def state(torch_cuda):
    from sos_amd import shmem as S
    S.lib()
    torch = torch_cuda
    one, two, full = grid_sizes(S)
    n = full + 64
    pool = np.frombuffer(bytearray(np.random.default_rng(0x516).bytes(n)), dtype=np.uint8)
    return {"S": S, "torch": torch, "pool": pool, "src": torch.from_numpy(pool).cuda(),
            "dst": torch.empty(GUARD + 16 + n + GUARD, dtype=torch.uint8, device="cuda"),
            "sig": torch.zeros(4, dtype=torch.int64, device="cuda"), "sum": 0, "sizes": (one, two, full)}


def run_case(st, n, dmis, smis, op, value):
    S, torch = st["S"], st["torch"]
    total = GUARD + dmis + n + GUARD
    dst = st["dst"][:total]
    dst.fill_(CANARY)
    assert st["src"].data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and smis + n <= st["pool"].size
    sig = st["sig"].data_ptr() + 8
    rc = S.sosx_put_signal(dst.data_ptr() + GUARD + dmis, st["src"].data_ptr() + smis, n, sig, value, op, None)
    assert rc == 0, (n, dmis, smis, op, rc)
    torch.cuda.synchronize()
    st["sum"] = value if op == SET else (st["sum"] + value) & (2**64 - 1)
    got = dst.cpu().numpy()
    exp = np.full(total, CANARY, dtype=np.uint8)
    exp[GUARD + dmis:GUARD + dmis + n] = st["pool"][smis:smis + n]
    bad = np.flatnonzero(got != exp)
    where = f"n={n} dmis={dmis} smis={smis} op={op} plan={plan(S, dst.data_ptr() + GUARD + dmis, st['src'].data_ptr() + smis, n)}"
    assert bad.size == 0, f"{where}: {bad.size} bytes differ, first at {bad[0] - GUARD - dmis}"
    words = st["sig"].cpu().numpy().view(np.uint64)
    assert int(words[1]) == st["sum"] and int(words[0]) == 0 and int(words[2]) == 0, (where, words, st["sum"])
    ticket = S.sosx_put_signal_ticket()
    assert ticket
    t = torch.zeros(1, dtype=torch.int32)
    copy = S.lib().sosx_memcpy
    copy.restype, copy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert copy(t.data_ptr(), ticket, 4, None) == 0
    assert int(t[0]) == 0, (where, int(t[0]))


def test_all_residues_at_a_small_size(state):
    k = 0
    for dmis in range(16):
        for smis in range(16):
            k += 1
            run_case(state, 61, dmis, smis, ADD if k % 2 else SET, 0x1000000000 + k)


@pytest.mark.parametrize("n", FIXED)
def test_sizes_around_the_vector_and_the_tile(state, n):
    for i, (dmis, smis) in enumerate(PAIRS):
        run_case(state, n, dmis, smis, SET if i % 2 else ADD, 7 + n + i)


def test_sizes_at_which_the_grid_changes(state):
    S = state["S"]
    one, two, full = state["sizes"]
    a, b = 1 << 30, 1 << 31
    assert plan(S, a, b, one)[6] == 1 and plan(S, a, b, two)[6] == 2 and two == one + 1
    assert plan(S, a, b, full)[6] == plan(S, a, b, full)[7] > plan(S, a, b, full - 1)[6]
    for n in (one, two, full):
        for i, (dmis, smis) in enumerate(PAIRS):
            run_case(state, n, dmis, smis, ADD if i % 2 else SET, (1 << 63) + n + i)   # ADD wraps past 2^64


def test_add_accumulates_and_set_replaces(state):
    run_case(state, 0, 0, 0, SET, 5)
    run_case(state, 0, 0, 0, ADD, 2**64 - 1)   # 5 + (2^64 - 1) wraps to 4
    assert state["sum"] == 4
    run_case(state, 24, 8, 8, ADD, 3)
    assert state["sum"] == 7


def test_bad_arguments_are_refused_before_any_launch(state):
    S = state["S"]
    f = S.sosx_put_signal
    d, s, g = state["dst"].data_ptr(), state["src"].data_ptr(), state["sig"].data_ptr()
    assert f(d, s, 8, None, 1, SET, None) == ERR_ARG        # null sig_addr
    assert f(d, s, 8, g + 4, 1, SET, None) == ERR_ARG       # misaligned sig_addr
    assert f(d, s, 8, g, 1, 2, None) == ERR_ARG             # unknown sig_op
    assert f(d, s, 8, g, 1, -1, None) == ERR_ARG
    assert f(None, s, 8, g, 1, SET, None) == ERR_ARG        # null target with bytes to move
    assert f(d, None, 8, g, 1, SET, None) == ERR_ARG        # null source
    state["torch"].cuda.synchronize()
    assert state["sig"].cpu().numpy().view(np.uint64)[0] == 0
