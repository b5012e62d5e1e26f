"""CPU: sos_sync_eval (onesided_checks.cpp), the comparison of a wait or test over a snapshot
of its ivars, against a short Python model written from SOS's macros (SHMEM_TEST and the
loops of src/synchronization_c.c4): all six comparisons x widths 2 / 4 / 8 x signed /
unsigned with values at the sign boundary, status NULL / all-masked / partly masked, nelems
0, 1 and 65, scalar and vector values, the `any` index and the `some` list and count."""
import ctypes
import itertools
import operator

import pytest

from sos_amd import shmem as S

ONE, ALL, ANY, SOME = range(4)
SIZE_MAX = 2**64 - 1
CMP = {1: operator.eq, 2: operator.ne, 3: operator.gt, 4: operator.ge, 5: operator.lt, 6: operator.le}
CTYPES = {(2, 1): ctypes.c_int16, (2, 0): ctypes.c_uint16, (4, 1): ctypes.c_int32, (4, 0): ctypes.c_uint32,
          (8, 1): ctypes.c_int64, (8, 0): ctypes.c_uint64}


def boundary(width, signed):
    bits = 8 * width
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    return [0, 1, lo, hi, -1 if signed else hi - 1, lo + 1, 42]


def model(words, status, cmp, values, kind):
    """(satisfied, any index, some indices) as SOS's loops compute them, `any` from index 0."""
    live = [i for i in range(len(words)) if not (status and status[i])]
    hold = [i for i in live if CMP[cmp](words[i], values[i])]
    if not live:
        return 1, SIZE_MAX, []
    ok = len(hold) == len(live) if kind in (ONE, ALL) else bool(hold)
    return int(ok), (hold[0] if hold and kind == ANY else SIZE_MAX), (hold if kind == SOME else [])


def run(words, width, signed, status, cmp, values, vector, kind):
    ct = CTYPES[(width, signed)]
    n = len(words)
    w = (ct * max(n, 1))(*words)
    v = (ct * max(n, 1))(*(values if vector else values[:1]))
    st = (ctypes.c_int * max(n, 1))(*status) if status is not None else None
    idx, cnt = ctypes.c_size_t(77), ctypes.c_size_t(77)
    indices = (ctypes.c_size_t * max(n, 1))(*([99] * max(n, 1)))
    r = S.sos_sync_eval(w, n, width, signed, st, cmp, v, vector, kind, ctypes.byref(idx), indices, ctypes.byref(cnt))
    return r, idx.value, list(indices)[:cnt.value], cnt.value


@pytest.mark.parametrize("width,signed", list(CTYPES))
def test_eval_matches_the_model(width, signed):
    pool = boundary(width, signed)
    ran = 0
    for n in (0, 1, 65):
        for rot, cmp, mask, vector in itertools.product(range(len(pool)), CMP, ("null", "none", "part", "all"), (0, 1)):
            words = [pool[(i + rot) % len(pool)] for i in range(n)]
            values = [pool[(3 * i + rot + 1) % len(pool)] for i in range(max(n, 1))]
            status = {"null": None, "none": [0] * n, "part": [int((i + rot) % 3 == 0) for i in range(n)], "all": [1] * n}[mask]
            for kind in (ONE, ALL, ANY, SOME):
                if kind == ONE and (n != 1 or status is not None):
                    continue
                vals = values if vector else [values[0]] * max(n, 1)
                want = model(words, status, cmp, vals, kind)
                r, idx, some, cnt = run(words, width, signed, status, cmp, values, vector, kind)
                assert (r, idx, some) == want and cnt == len(want[2]), (n, rot, cmp, mask, vector, kind, words[:4], vals[:4])
                ran += 1
    # three kinds at each of the three sizes, ONE for n = 1 and status NULL
    assert ran == len(pool) * 6 * 4 * 2 * (3 + 3 + 3) + len(pool) * 6 * 2


def test_a_short_of_minus_one_is_not_65535():
    assert run([-1], 2, 1, None, 5, [0], 0, ONE)[0] == 1            # -1 < 0
    assert run([65535], 2, 0, None, 5, [0], 0, ONE)[0] == 0         # 65535 < 0 is false
    assert run([-1], 2, 1, None, 3, [32767], 0, ONE)[0] == 0        # -1 > SHRT_MAX is false
    assert run([-2**31], 4, 1, None, 5, [2**31 - 1], 0, ONE)[0] == 1
    assert run([2**63], 8, 0, None, 3, [2**63 - 1], 0, ONE)[0] == 1  # unsigned: above the signed range
    assert run([-2**63], 8, 1, None, 3, [2**63 - 1], 0, ONE)[0] == 0


def test_empty_and_masked_give_soss_return_values():
    for kind in (ALL, ANY, SOME):
        assert run([], 8, 0, None, 1, [1], 0, kind) == (1, SIZE_MAX, [], 0)
        assert run([5, 6], 8, 0, [1, 1], 1, [5], 0, kind) == (1, SIZE_MAX, [], 0)
    # test_some reports whatever holds in one pass; any gives the lowest satisfied unmasked index
    assert run([7, 0, 7, 7], 4, 1, [0, 0, 1, 0], 1, [7], 0, SOME) == (1, SIZE_MAX, [0, 3], 2)
    assert run([0, 7, 7, 7], 4, 1, [0, 1, 0, 0], 1, [7], 0, ANY) == (1, 2, [], 0)
    assert run([0, 7, 0, 0], 4, 1, [0, 1, 0, 0], 1, [7], 0, ANY) == (0, SIZE_MAX, [], 0)


def test_unusable_arguments():
    f = S.sos_sync_eval
    w = (ctypes.c_int64 * 2)(1, 2)
    idx, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    args = lambda **k: [k.get("w", w), k.get("n", 2), k.get("width", 8), 1, None, k.get("cmp", 1), k.get("v", w), 0,  # noqa: E731
                        k.get("kind", ALL), ctypes.byref(idx), k.get("indices", None), ctypes.byref(cnt)]
    assert f(*args()) in (0, 1)
    assert f(*args(width=1)) == -1 and f(*args(width=16)) == -1
    assert f(*args(cmp=0)) == -1 and f(*args(cmp=7)) == -1
    assert f(*args(kind=4)) == -1 and f(*args(kind=ONE)) == -1        # ONE takes exactly one word
    assert f(*args(w=None)) == -1 and f(*args(v=None)) == -1
    assert f(*args(kind=SOME)) == -1                                   # nowhere to put the indices
