"""GPU: the fcollect and alltoall plans run by the single-GPU loopback executor (P PEs'
buffers on one device), against the closed forms of SOS's block placement
(src/collectives.c:1284-1480):

  fcollect:  target of every PE = concat over q of source(q)
  alltoall:  target(i) block j  = source(j) block i
"""
import numpy as np
import pytest

from sos_amd import _lib
from sos_amd import shmem as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3
TAIL = 16
# (datatype, per-PE / per-pair block in bytes)
SHAPES = [("uchar", 1), ("uchar", 1000), ("uchar", 65536 + 4), ("uint64", (1 << 20) + 8)]


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 12])
@pytest.mark.parametrize("alg", ["fcollect", "alltoall"])
def test_collect_loopback(torch_cuda, alg, P, shape, pad):
    torch = torch_cuda
    dt, B = shape
    es = 8 if dt == "uint64" else 1
    count = B // es
    sb, db = _lib.plan_extents(alg, P, count, es)
    assert (sb, db) == ((B if alg == "fcollect" else P * B), P * B)
    rng = np.random.default_rng(97 * P + B)
    srcs = [rng.integers(0, 256, sb, dtype=np.uint8) for _ in range(P)]
    ds = []
    for a in srcs:
        t = torch.empty(pad + sb, dtype=torch.uint8, device="cuda")
        t[pad:] = torch.from_numpy(a).cuda()
        ds.append(t)
    dd = [torch.full((pad + db + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(P)]
    S.loopback_allreduce(alg, "sum", dt, [t.data_ptr() + pad for t in ds],
                         [t.data_ptr() + pad for t in dd], count)
    torch.cuda.synchronize()
    if alg == "fcollect":
        exp = [np.concatenate(srcs)] * P
    else:
        exp = [np.concatenate([srcs[j][i * B:(i + 1) * B] for j in range(P)]) for i in range(P)]
    for p in range(P):
        got = dd[p].cpu().numpy()
        assert np.all(got[:pad] == SENTINEL), f"PE {p}: bytes before the target changed"
        assert np.array_equal(got[pad:pad + db], exp[p]), f"{alg} P={P} B={B} pad={pad}: PE {p} differs"
        assert np.all(got[pad + db:] == SENTINEL), f"PE {p}: bytes after the target changed"
        assert np.array_equal(ds[p].cpu().numpy()[pad:], srcs[p]), f"PE {p}: source changed"


def test_collect_loopback_count_zero_and_bad_type(torch_cuda):
    torch = torch_cuda
    t = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    for alg in ("fcollect", "alltoall"):
        S.loopback_allreduce(alg, "sum", "uchar", [t.data_ptr()] * 2, [t.data_ptr() + 32] * 2, 0)
        with pytest.raises(_lib.SosError):
            S.loopback_allreduce(alg, "sum", 99, [t.data_ptr()] * 2, [t.data_ptr() + 32] * 2, 1)
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all())
