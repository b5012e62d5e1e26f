"""GPU: all P collect plans run by the single-GPU loopback executor (P PEs' buffers on one
device), against a plain concatenation of seeded per-PE byte arrays
(src/collectives.c:1215-1276: the target of every PE = concat over q of source(q))."""
import numpy as np
import pytest

from sos_amd import shmem as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3
TAIL = 64
ODD = (1, 3, 15, 17, 255)


def length_vectors(P):
    v = {"equal": [1000] * P, "zero": [0] * P, "one": [0] * (P - 1) + [255],
         "alternating": [0 if q % 2 == 0 else ODD[(q // 2) % len(ODD)] for q in range(P)],
         "long_among_short": [1 + q % 3 for q in range(P)],
         "zero_first_last": [0] + [16 * q + 1 for q in range(1, P - 1)] + [0]}
    v["long_among_short"][P // 2] = (1 << 20) + 3
    return v


@pytest.mark.parametrize("heap", [False, True], ids=["separate", "heap"])
@pytest.mark.parametrize("name", ["equal", "zero", "one", "alternating", "long_among_short",
                                  "zero_first_last"])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_collectv_loopback(torch_cuda, P, name, heap):
    """heap: every PE's source and target are carved, at odd offsets, out of one
    allocation (the layout of a symmetric heap); otherwise each is its own allocation."""
    torch = torch_cuda
    lens = length_vectors(P)[name]
    total = sum(lens)
    rng = np.random.default_rng(131 * P + total)
    srcs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    if heap:
        pad = 5
        sslot = (max(lens) + pad + 63) // 64 * 64 + 64
        dslot = (pad + total + TAIL + 63) // 64 * 64 + 64
        arena = torch.full((P * (sslot + dslot),), SENTINEL, dtype=torch.uint8, device="cuda")
        ds = [arena[p * sslot:(p + 1) * sslot] for p in range(P)]
        dd = [arena[P * sslot + p * dslot:P * sslot + (p + 1) * dslot] for p in range(P)]
    else:
        pad = 0
        ds = [torch.full((pad + n + 1,), SENTINEL, dtype=torch.uint8, device="cuda") for n in lens]
        dd = [torch.full((pad + total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(P)]
    for t, a in zip(ds, srcs):
        if a.size:
            t[pad:pad + a.size] = torch.from_numpy(a).cuda()
    S.loopback_collect([t.data_ptr() + pad for t in ds], [t.data_ptr() + pad for t in dd], lens)
    torch.cuda.synchronize()
    exp = np.concatenate(srcs)
    for p in range(P):
        got = dd[p].cpu().numpy()
        assert np.all(got[:pad] == SENTINEL), f"PE {p}: bytes before the target changed"
        assert np.array_equal(got[pad:pad + total], exp), f"collect P={P} {name}: PE {p} differs"
        assert np.all(got[pad + total:] == SENTINEL), f"PE {p}: bytes above the sum changed"
        assert np.array_equal(ds[p].cpu().numpy()[pad:pad + lens[p]], srcs[p]), f"PE {p}: source changed"


def test_collectv_loopback_null_source_for_zero_length(torch_cuda):
    torch = torch_cuda
    s = torch.arange(7, dtype=torch.uint8, device="cuda")
    dd = [torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    S.loopback_collect([None, s.data_ptr()], [t.data_ptr() for t in dd], [0, 7])
    torch.cuda.synchronize()
    for t in dd:
        assert t.cpu().numpy().tolist() == list(range(7)) + [SENTINEL] * 9
