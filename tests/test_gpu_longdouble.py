"""GPU: directed long double vectors through every kernel family that instantiates ld80.

The encodings of tests/ldbl_vectors.py (a subset of the list tests/test_ldbl_x87.py runs
on the host: unnormals, pseudo-NaN / pseudo-infinity / pseudo-denormals, quiet and
signalling NaN payloads of both signs, exact rounding ties, the carry out of 64 bits, the
step into the smallest normal, overflow by rounding, padding bytes that differ between
the operands) go through the combine, the fold in both orders, the prefix, the small
host-resident path and the loopback ring / recdbl.  The reference is the oracle on this
machine's own x87 (reduce_local, the plan simulator's fold, ring, recdbl); all 16 bytes
of every element must agree, NaNs included.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from sos_amd import _lib, shmem as S

import ldbl_vectors as V
import plansim
from test_gpu_collectives import _pinned, cpu_prefix, from_dev, to_dev

pytestmark = pytest.mark.gpu

LD = 25
OPS = [3, 4, 5, 6]  # min, max, sum, prod


def assert_same(got, ref, what, ins=()):
    bad = V.bad_rows(got, ref)
    assert bad.size == 0, (what, f"{bad.size} of {got.size} elements differ",
                           [(int(i), [V.show(x, i) for x in ins], V.show(got, i), V.show(ref, i)) for i in bad[:4]])


@functools.lru_cache(maxsize=None)
def pairs():
    return V.all_pairs()


@functools.lru_cache(maxsize=None)
def pairs_ref(op):
    a, b = pairs()
    ref = a.copy()
    O.reduce_local(op, LD, b, ref)
    return ref


@functools.lru_cache(maxsize=None)
def permuted(P, n):
    return V.permuted_inputs(P, n, seed=P)


@pytest.mark.parametrize("op", OPS)
def test_combine_all_pairs(torch_cuda, op):
    """sosx_combine on every ordered pair of the encodings; then from the second element
    (+16 B) over a ragged length."""
    torch = torch_cuda
    a, b = pairs()
    ref = pairs_ref(op)
    n = a.size
    assert 700000 < n < (1 << 20)
    da, db = to_dev(torch, a), to_dev(torch, b)
    _lib.combine(op, LD, da.data_ptr(), db.data_ptr(), n)
    torch.cuda.synchronize()
    assert_same(from_dev(da, a), ref, ("combine", op), (a, b))
    m = n - 1 - 4093
    da = to_dev(torch, a)
    _lib.combine(op, LD, da.data_ptr() + 16, db.data_ptr() + 16, m)
    torch.cuda.synchronize()
    exp = a.copy()
    exp[1:1 + m] = ref[1:1 + m]
    assert_same(from_dev(da, a), exp, ("combine +16 B ragged", op), (a, b))


@pytest.mark.parametrize("op", OPS)
def test_combine3_all_pairs(torch_cuda, op):
    """sosx_combine3 (out of place): the same pairs, the inputs left as they were."""
    torch = torch_cuda
    a, b = pairs()
    ref = pairs_ref(op)
    n = a.size
    da, db = to_dev(torch, a), to_dev(torch, b)
    out = torch.full_like(da, 0xA5)
    _lib.combine3(op, LD, out.data_ptr(), da.data_ptr(), db.data_ptr(), n)
    torch.cuda.synchronize()
    assert_same(from_dev(out, a), ref, ("combine3", op), (a, b))
    assert_same(from_dev(da, a), a, "combine3 input a")
    assert_same(from_dev(db, b), b, "combine3 input b")
    m = n - 1 - 4093
    out = torch.full_like(da, 0xA5)
    _lib.combine3(op, LD, out.data_ptr() + 16, da.data_ptr() + 16, db.data_ptr() + 16, m)
    torch.cuda.synchronize()
    got = from_dev(out, a)
    assert_same(got[1:1 + m], ref[1:1 + m], ("combine3 +16 B ragged", op), (a[1:], b[1:]))
    raw = got.view(np.uint8)
    assert (raw[:16] == 0xA5).all() and (raw[16 * (1 + m):] == 0xA5).all()


# 4096 long doubles are 64 KiB per input: the last length of the small-input fold
# (k_fold_dyn), 4097 the first of the streaming one; runtime-P folds (P > 8) at n = 1000
FOLD_CASES = [(P, n) for P in (2, 3, 5, 8) for n in (4096, 4097)] + [(P, 1000) for P in (9, 12, 64)]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P,n", FOLD_CASES)
def test_fold_permuted(torch_cuda, P, n, order):
    """sosx_fold in the ring's LINEAR and recdbl_sw's TREE order: input k is the encoding
    list under permutation k."""
    torch = torch_cuda
    ins = permuted(P, n)
    di = [to_dev(torch, x) for x in ins]
    for op in OPS:
        ref = plansim.fold_values(op, LD, ins, order)
        out = torch.zeros_like(di[0])
        _lib.fold(op, LD, order, out.data_ptr(), [t.data_ptr() for t in di], n)
        torch.cuda.synchronize()
        assert_same(from_dev(out, ref), ref, ("fold", P, n, order, op), ins)


@pytest.mark.parametrize("op", [5, 6, 3])
@pytest.mark.parametrize("np_", [2, 8, 12])
def test_prefix_permuted(torch_cuda, np_, op):
    """sosx_prefix: outs[k] = ins[0] OP ... OP ins[k], the running value the left operand."""
    torch = torch_cuda
    n = 2525
    ins = permuted(np_, n)
    ref = cpu_prefix(op, LD, ins)
    di = [to_dev(torch, x) for x in ins]
    do = [torch.zeros_like(t) for t in di]
    _lib.prefix(op, LD, [t.data_ptr() for t in do], [t.data_ptr() for t in di], n)
    torch.cuda.synchronize()
    for k in range(np_):
        assert_same(from_dev(do[k], ref[k]), ref[k], ("prefix", np_, op, k), ins[:k + 1])


def _small_setup(torch, srcs):
    """Pinned host copies of the operands, a pinned result and the completion words."""
    keep = [_pinned(torch, np.frombuffer(a.tobytes(), np.uint8), 0) for a in srcs]
    ob, optr = _pinned(torch, np.full(srcs[0].nbytes, 0xA5, np.uint8), 0)
    flags = torch.zeros(4096 + 8, dtype=torch.int32, pin_memory=True)
    return keep, [q for _, q in keep], ob, optr, flags


def _small_result(ob, optr, like):
    off = optr - ob.data_ptr()
    return np.frombuffer(ob[off:off + like.nbytes].numpy().tobytes(), like.dtype)


SMALL_P = 4
SMALL_N = (7, 1683)


@pytest.mark.parametrize("op", OPS)
def test_small_fold_permuted(torch_cuda, op):
    """sosx_small_fold at P = 4: every PE's own recdbl_sw value (oracle recdbl, per PE)."""
    torch = torch_cuda
    L = _lib.lib()
    P = SMALL_P
    seq = 0
    for n in SMALL_N:
        srcs = permuted(P, n)
        ref = O.recdbl(op, LD, srcs)
        keep, ptr, ob, optr, flags = _small_setup(torch, srcs)
        for me in range(P):
            leaves = [ptr[y ^ me] for y in range(P)]
            seq += 1
            ob.fill_(0xA5)
            nb = ctypes.c_int(-1)
            rc = L.sosx_small_fold(op, LD, ctypes.c_void_p(optr), (ctypes.c_void_p * P)(*leaves),
                                   (ctypes.c_void_p * P)(*([None] * P)), P, ctypes.c_size_t(n),
                                   ctypes.c_void_p(flags.data_ptr()), ctypes.c_uint32(seq), ctypes.byref(nb), None)
            assert rc == 0
            torch.cuda.synchronize()
            assert bool((flags[:nb.value] == seq).all())
            assert_same(_small_result(ob, optr, srcs[0]), ref[me], ("small_fold", op, n, me), srcs)


@pytest.mark.parametrize("op", OPS)
def test_small_ring_permuted(torch_cuda, op):
    """sosx_small_ring at P = 4: SOS's ring result (chunk c folded from PE c)."""
    torch = torch_cuda
    L = _lib.lib()
    P = SMALL_P
    for seq, n in enumerate(SMALL_N, 1):
        srcs = permuted(P, n)
        ref = O.ring(op, LD, srcs)
        keep, ptr, ob, optr, flags = _small_setup(torch, srcs)
        nb = ctypes.c_int(-1)
        rc = L.sosx_small_ring(op, LD, ctypes.c_void_p(optr), (ctypes.c_void_p * P)(*ptr), P, ctypes.c_size_t(n),
                               ctypes.c_void_p(flags.data_ptr()), ctypes.c_uint32(seq), ctypes.byref(nb), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((flags[:nb.value] == seq).all())
        got = _small_result(ob, optr, srcs[0])
        for p in range(P):
            assert_same(got, ref[p], ("small_ring", op, n, p), srcs)


@pytest.mark.parametrize("op", OPS)
def test_small_linear_permuted(torch_cuda, op):
    """sosx_small_linear at np = 4: the in-order fold, the running value the left operand."""
    torch = torch_cuda
    L = _lib.lib()
    P = SMALL_P
    for seq, n in enumerate(SMALL_N, 1):
        srcs = permuted(P, n)
        ref = cpu_prefix(op, LD, srcs)[-1]
        keep, ptr, ob, optr, flags = _small_setup(torch, srcs)
        nb = ctypes.c_int(-1)
        rc = L.sosx_small_linear(op, LD, ctypes.c_void_p(optr), (ctypes.c_void_p * P)(*ptr), P, ctypes.c_size_t(n),
                                 ctypes.c_void_p(flags.data_ptr()), ctypes.c_uint32(seq), ctypes.byref(nb),
                                 seq % 2, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((flags[:nb.value] == seq).all())
        assert_same(_small_result(ob, optr, srcs[0]), ref, ("small_linear", op, n), srcs)


@pytest.mark.parametrize("alg", ["ring", "recdbl"])
@pytest.mark.parametrize("P", [3, 5])
def test_loopback_permuted(torch_cuda, alg, P):
    """The loopback ring and recdbl plans against SOS's schedules, per PE."""
    torch = torch_cuda
    n = 2525
    srcs = permuted(P, n)
    ds = [to_dev(torch, x) for x in srcs]
    for op in OPS:
        ref = (O.ring if alg == "ring" else O.recdbl)(op, LD, srcs)
        dd = [torch.zeros_like(t) for t in ds]
        S.loopback_allreduce(alg, op, LD, [t.data_ptr() for t in ds], [t.data_ptr() for t in dd], n)
        torch.cuda.synchronize()
        for p in range(P):
            assert_same(from_dev(dd[p], srcs[p]), ref[p], ("loopback", alg, P, op, p), srcs)
