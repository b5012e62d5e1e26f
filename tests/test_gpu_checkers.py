"""GPU: the suite's own device-side checkers.

sosx_count_mismatch (synth.hip k_mismatch) is the verdict of the signal ping-pong, of the
team benchmark's preflight and of the benchmark's self-check: here its count is compared
with a numpy count of the elements whose bytes differ, for differences planted where a
counting kernel goes wrong -- the first and the last element, both sides of every wave and
workgroup boundary, two words of one element, an element's top byte -- at every word
width, on and off alignment, and past the grid cap.  sosx_fill generates the inputs of the
multi-PE tests and the benchmark: bit for bit against oracle.fill for every kind the
kernel's switch distinguishes, at element indices past 2^32 and past the grid cap.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = (1 << 21) + 257  # past k_mismatch's 8192 x 256 grid: the stride loop repeats


def planted(n, es):
    """{name: (element indices, byte-within-element indices)} of the bytes to flip."""
    mid = n // 2
    edges = np.unique(np.concatenate([np.arange(63, n, 64), np.arange(64, n, 64)])).astype(np.int64)
    every = np.arange(n, dtype=np.int64)
    return {
        "none": (np.zeros(0, np.int64), np.zeros(0, np.int64)),
        "first": (np.array([0]), np.array([0])),
        "last": (np.array([n - 1]), np.array([es - 1])),
        "boundaries": (edges, edges % es),
        "two_words_one_element": (np.array([mid, mid]), np.array([0, es - 1])),
        "top_byte": (np.array([mid]), np.array([es - 1])),
        "every": (every, every % es),
    }


@pytest.mark.parametrize("es", [1, 2, 3, 4, 8, 12, 16, 32])
def test_count_mismatch(torch_cuda, sos, es):
    torch = torch_cuda
    rng = np.random.default_rng(es)
    counts = [1, 63, 64, 65, 255, 256, 257] + ([BIG] if es in (1, 4) else [])
    for n in counts:
        a = rng.integers(0, 256, n * es, dtype=np.uint8)
        for off in (0, 1):  # 1: no word but the byte is aligned
            da = torch.zeros(n * es + 16, dtype=torch.uint8, device="cuda")
            db = torch.zeros(n * es + 16, dtype=torch.uint8, device="cuda")
            assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
            da[off:off + n * es].copy_(torch.from_numpy(a))
            for name, (elems, inner) in planted(n, es).items():
                b = a.copy()
                at = elems * es + inner
                b[at] = b[at] ^ 0x80  # (a byte named twice, es == 1, is flipped once)
                want = int(np.count_nonzero((a.reshape(n, es) != b.reshape(n, es)).any(axis=1)))
                if name == "every":
                    assert want == n
                elif name in ("first", "last", "top_byte"):
                    assert want == 1
                db[off:off + n * es].copy_(torch.from_numpy(b))
                torch.cuda.synchronize()
                got = sos.count_mismatch(da.data_ptr() + off, db.data_ptr() + off, n, es)
                assert got == want, (es, n, off, name, got, want)


def test_count_mismatch_status_codes(torch_cuda, sos):
    torch = torch_cuda
    L = sos.lib()
    a = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = ctypes.c_ulonglong(99)
    assert L.sosx_count_mismatch(a.data_ptr(), a.data_ptr(), 0, 4, ctypes.byref(out), None) == 0
    assert out.value == 0
    out.value = 99
    assert L.sosx_count_mismatch(None, None, 0, 4, ctypes.byref(out), None) == 0 and out.value == 0
    assert L.sosx_count_mismatch(a.data_ptr(), a.data_ptr(), 16, 4, None, None) == -3
    assert L.sosx_count_mismatch(a.data_ptr(), a.data_ptr(), 16, 0, ctypes.byref(out), None) == -3


# one datatype of every kind synth.hip's switch distinguishes: float, double, both complex
# types, and integers of 1, 2, 4 and 8 bytes (signed and unsigned share a kernel: both run)
FILL_KINDS = {"schar": 2, "uchar": 13, "short": 3, "ushort": 14, "int": 4, "uint": 15, "long": 5, "ulong": 16,
              "float": 23, "double": 24, "complexf": 26, "complexd": 27}
FILL_BIG = 4 * (1 << 20) + 257  # past k_fill's 16384 x 256 grid


@pytest.mark.parametrize("name", list(FILL_KINDS))
def test_fill_kinds_match_oracle(torch_cuda, sos, oracle, name):
    torch = torch_cuda
    dt = FILL_KINDS[name]
    es = np.dtype(oracle.np_type(dt)).itemsize
    sizes = [10007] + ([FILL_BIG] if es in (1, 4) else [])
    for n in sizes:
        for dist in (0, 1):
            for index0 in (0, (1 << 33) + 5):
                ref = oracle.fill(dt, dist, 4321, 2, n, index0)
                buf = torch.full((ref.nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                sos.fill(dt, dist, 4321, 2, buf.data_ptr(), n, index0)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                assert np.array_equal(got[:ref.nbytes], np.frombuffer(ref.tobytes(), np.uint8)), \
                    (name, n, dist, index0)
                assert (got[ref.nbytes:] == 0xA5).all(), (name, n, dist, index0)


def test_fill_status_codes(torch_cuda, sos):
    L = sos.lib()
    buf = torch_cuda.zeros(64, dtype=torch_cuda.uint8, device="cuda")
    assert L.sosx_fill(25, 0, 1, 0, buf.data_ptr(), 4, 0, None) == -6   # long double: SOSX_ERR_UNSUPPORTED
    assert L.sosx_fill(28, 0, 1, 0, buf.data_ptr(), 4, 0, None) == -1   # no such datatype: SOSX_ERR_DTYPE
    assert L.sosx_fill(-1, 0, 1, 0, buf.data_ptr(), 4, 0, None) == -1
    assert L.sosx_fill(0, 0, 1, 0, buf.data_ptr(), 4, 0, None) == -1    # SIGNED_BYTE: not a SOS reduction type
    assert L.sosx_fill(23, 0, 1, 0, None, 0, 0, None) == 0              # nothing to fill
    assert L.sosx_fill(23, 0, 1, 0, None, 4, 0, None) == -3
    torch_cuda.cuda.synchronize()
    assert not bool(buf.any())
