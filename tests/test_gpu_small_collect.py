"""GPU: sosx_small_collect alone in one process -- the one launch that concatenates up to
64 segments of arbitrary byte lengths (collect's small path, sos_amd/csrc/small.hip)
-- against numpy's concatenation: destinations at every kind of misalignment with
canaries on both sides, sources at mixed offsets (aligned, on the 4-B grid, odd), the
completion words, and the argument checks that answer before any launch."""
import ctypes

import numpy as np
import pytest

from sos_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 256 * 4 * 16          # kThreads * kCollectU vectors of 16 B
POOL = [0, 1, 15, 16, 17, 255, TILE - 1, TILE, TILE + 1, (64 << 10) + 3]
CANARY = 64
SRC_OFFS = (0, 4, 1, 8, 3, 12, 15, 2)
SEQ = 0x5EED0001


def vectors(np_):
    rng = np.random.default_rng(7 * np_)
    v = {"pool": [POOL[(3 * q + np_) % len(POOL)] for q in range(np_)],
         "random": [int(POOL[i]) for i in rng.integers(0, len(POOL), np_)],
         "all_zero": [0] * np_}
    if np_ >= 3:
        v["zero_ends"] = [0] + [POOL[1 + q % (len(POOL) - 1)] for q in range(np_ - 2)] + [0]
    return v


def run(torch, lens, out_off):
    L = _lib.lib()
    np_ = len(lens)
    total = sum(lens)
    rng = np.random.default_rng(1000 * np_ + total + out_off)
    srcs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    dev, ptrs = [], []
    for q, a in enumerate(srcs):
        so = SRC_OFFS[q % len(SRC_OFFS)]
        t = torch.zeros(so + a.size + 16, dtype=torch.uint8, device="cuda")
        if a.size:
            t[so:so + a.size] = torch.from_numpy(a).cuda()
        dev.append(t)
        ptrs.append(t.data_ptr() + so if a.size else None)
    out = torch.full((CANARY + 16 + total + CANARY,), 0xC3, dtype=torch.uint8, device="cuda")
    base = (out.data_ptr() + CANARY + 15) // 16 * 16 + out_off  # 16-B aligned + the asked offset
    lo = base - out.data_ptr()
    nflags = np_ + total // (16 << 10) + 1
    flags = torch.zeros(nflags + 4, dtype=torch.int32, device="cuda")
    nb = ctypes.c_int(-1)
    segs = (ctypes.c_void_p * np_)(*ptrs)
    n = (ctypes.c_size_t * np_)(*lens)
    torch.cuda.synchronize()
    rc = L.sosx_small_collect(base, segs, n, np_, flags.data_ptr(), SEQ, ctypes.byref(nb), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exp = np.concatenate(srcs) if total else np.zeros(0, np.uint8)
    assert np.all(got[:lo] == 0xC3), "bytes below the target changed"
    assert np.array_equal(got[lo:lo + total], exp), f"np={np_} lens={lens[:6]} out_off={out_off}"
    assert np.all(got[lo + total:] == 0xC3), "bytes above the sum changed"
    f = flags.cpu().numpy().view(np.uint32)
    assert 0 <= nb.value <= nflags and (nb.value == 0) == (total == 0)
    assert np.all(f[:nb.value] == SEQ) and np.all(f[nb.value:] == 0), "completion words"
    for t, a, q in zip(dev, srcs, range(np_)):
        so = SRC_OFFS[q % len(SRC_OFFS)]
        assert np.array_equal(t.cpu().numpy()[so:so + a.size], a), "a source changed"


@pytest.mark.parametrize("out_off", [0, 1, 4, 15])
@pytest.mark.parametrize("np_", [1, 2, 3, 8, 17, 64])
def test_small_collect(torch_cuda, np_, out_off):
    for lens in vectors(np_).values():
        run(torch_cuda, lens, out_off)


def test_small_collect_every_pool_length_alone(torch_cuda):
    """np = 1: each pool length through each source misalignment class (SRC_OFFS[0] = 0
    here, so shift the target instead: the incongruence is what selects the load form)."""
    for n in POOL:
        for out_off in (0, 1, 4, 15):
            run(torch_cuda, [n], out_off)


def test_small_collect_rejects_bad_args_before_launch(torch_cuda):
    torch = torch_cuda
    L = _lib.lib()
    buf = torch.full((256,), 0xC3, dtype=torch.uint8, device="cuda")
    flags = torch.zeros(80, dtype=torch.int32, device="cuda")
    p, fp = buf.data_ptr(), flags.data_ptr()
    nb = ctypes.c_int(0)
    one = (ctypes.c_void_p * 1)(p + 128)
    nul = (ctypes.c_void_p * 1)(None)
    n4 = (ctypes.c_size_t * 1)(4)
    n0 = (ctypes.c_size_t * 1)(0)
    many = (ctypes.c_void_p * 65)(*([p + 128] * 65))
    nmany = (ctypes.c_size_t * 65)(*([1] * 65))
    f = L.sosx_small_collect
    assert f(p, one, n4, 0, fp, 1, ctypes.byref(nb), None) == -3
    assert f(p, many, nmany, 65, fp, 1, ctypes.byref(nb), None) == -3
    assert f(p, nul, n4, 1, fp, 1, ctypes.byref(nb), None) == -3      # null segment, length 4
    assert f(None, one, n4, 1, fp, 1, ctypes.byref(nb), None) == -3   # null target, sum 4
    assert f(p, None, n4, 1, fp, 1, ctypes.byref(nb), None) == -3
    assert f(p, one, None, 1, fp, 1, ctypes.byref(nb), None) == -3
    assert f(p, one, n4, 1, None, 1, ctypes.byref(nb), None) == -3
    assert f(p, one, n4, 1, fp, 1, None, None) == -3
    assert f(None, nul, n0, 1, fp, 1, ctypes.byref(nb), None) == 0 and nb.value == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool((buf == 0xC3).all()) and not bool(flags.any())
