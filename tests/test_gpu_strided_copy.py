"""GPU: sosx_strided_copy (the pack / unpack passes of shmem_alltoalls) against numpy
slicing, byte for byte, with every byte the copy must not touch checked: the gaps between
target elements, the bytes before the first element and the bytes after the last."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64  # bytes of sentinel kept before and after the target's extent
COUNTS = [1, 3, 15, 17, 255, 4099, 65536 + 5, (1 << 20) + 3]
STRIDES = [(1, 1), (1, 2), (1, 3), (3, 1), (2, 5), (7, 2), (1, 17)]
MAX_SRC = 16 * (((1 << 20) + 2) * 17 + 1) + 64


@pytest.fixture(scope="module")
def pool():
    """Random source bytes, generated once; every case reads a prefix of it."""
    return np.frombuffer(bytearray(np.random.default_rng(0x57D).bytes(MAX_SRC)), dtype=np.uint8)


def extent(count, stride, es):
    return es * ((count - 1) * stride + 1)


def elems(buf, count, stride, es):
    """(count, es) byte view of the elements `stride` elements apart in `buf` (no copy)."""
    assert buf.size == extent(count, stride, es)
    return np.lib.stride_tricks.as_strided(buf, shape=(count, es), strides=(stride * es, 1))


@pytest.mark.parametrize("strides", STRIDES, ids=lambda s: f"d{s[0]}s{s[1]}")
@pytest.mark.parametrize("es", [1, 2, 4, 8, 16])
def test_strided_copy_matches_numpy(torch_cuda, sos, pool, es, strides):
    torch = torch_cuda
    dstr, sst = strides
    # bases one and three elements past a 16-B boundary (element size 16: on the boundary)
    bases = [(0, 0)] if es == 16 else [(1, 3), (3, 1)]
    for count in COUNTS:
        sb, db = extent(count, sst, es), extent(count, dstr, es)
        for doff, soff in bases:
            doff, soff = doff * es, soff * es
            src_h = pool[:sb]
            src_d = torch.empty(soff + sb + 16, dtype=torch.uint8, device="cuda")
            src_d[soff:soff + sb] = torch.from_numpy(src_h).cuda()
            total = GUARD + doff + db + GUARD
            dst_d = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
            assert src_d.data_ptr() % 16 == 0 and dst_d.data_ptr() % 16 == 0
            sos.strided_copy(dst_d.data_ptr() + GUARD + doff, dstr, src_d.data_ptr() + soff, sst, es, count)
            torch.cuda.synchronize()
            got = dst_d.cpu().numpy()
            exp = np.full(total, SENTINEL, dtype=np.uint8)
            # element k of the source lands as element k of the target, strides in elements
            elems(exp[GUARD + doff:GUARD + doff + db], count, dstr, es)[:] = elems(src_h, count, sst, es)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (f"es={es} dst_stride={dstr} src_stride={sst} count={count} "
                                   f"bases=({doff},{soff}): {bad.size} bytes differ, first at "
                                   f"{bad[0] - GUARD - doff} of the target extent {db}")


@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_strided_copy_64bit_indexing(torch_cuda, sos, direction):
    """Element offsets beyond 2^32 bytes: 8-B elements (1 << 28) + 1 apart, the third one
    4 GiB + 16 B into an uninitialised allocation of which only three elements are used."""
    torch = torch_cuda
    stride = (1 << 28) + 1
    big = torch.empty((1 << 32) + 64, dtype=torch.uint8, device="cuda")
    big64 = big.view(torch.int64)
    idx = [k * stride for k in range(3)]
    assert idx[2] * 8 + 8 <= big.numel() and idx[2] * 8 > (1 << 32)
    vals = [0x0123456789ABCDEF, -0x0FEDCBA987654321, 0x5A5A5A5AA5A5A5A5]
    small = torch.full((3 + 2,), -1, dtype=torch.int64, device="cuda")  # one guard word each side
    if direction == "pack":
        for i, v in zip(idx, vals):
            big64[i] = v
        sos.strided_copy(small.data_ptr() + 8, 1, big.data_ptr(), stride, 8, 3)
        torch.cuda.synchronize()
        assert small.cpu().tolist() == [-1] + vals + [-1]
    else:
        small[1:4] = torch.tensor(vals, dtype=torch.int64)
        # neighbours of the three target elements must keep their bytes
        near = [i + d for i in idx for d in (-1, 1) if 0 <= i + d < big64.numel()]
        for i in near:
            big64[i] = 0x7777777777777777
        sos.strided_copy(big.data_ptr(), stride, small.data_ptr() + 8, 1, 8, 3)
        torch.cuda.synchronize()
        assert [int(big64[i]) for i in idx] == vals
        assert all(int(big64[i]) == 0x7777777777777777 for i in near)
