"""GPU: sosx_block_strided_copy (the data movement of shmemx_ibput / ibget and of
shmem_iput / iget) against numpy index arithmetic, byte for byte.  The target is filled
with a canary first and the WHOLE target buffer is compared: the blocks, the gaps between
them and a guard band before and after.

The cases are the CPU sweep of tests/blockcopy_plan.cpp (every element size; block sizes
around one and 64 16-B vectors; 1, 2, 3 and 257 blocks; strides equal to the block, one
more, a multiple of 16 B, 4099; base misalignments 0..15) thinned with a fixed seed to 40
per element size, plus one shape per regime whose grid has more than one workgroup.  The
smallest shapes are the ones that matter; none needs more than a few MiB."""
import ctypes
import itertools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64
PER_SIZE = 40
REGIMES = {1: "contiguous", 2: "element", 3: "small", 4: "congruent", 5: "incongruent"}


def sweep(es):
    V = 16 // es
    bsizes = sorted({1, 2, 3, V - 1, V, V + 1, 64 * V - 1, 64 * V, 64 * V + 5} - {0})
    out = []
    for bsize, nblocks in itertools.product(bsizes, (1, 2, 3, 257)):
        strides = (bsize, bsize + 1, (bsize // V + 2) * V, 4099)
        for dstr, sstr in itertools.product(strides, strides):
            if nblocks == 257 and es >= 8 and 4099 in (dstr, sstr):
                continue  # 8-17 MiB operands: the same paths run at the smaller element sizes
            for dmis, smis in itertools.product(range(0, 16, es), range(0, 16, es)):
                out.append((es, bsize, nblocks, dstr, sstr, dmis, smis))
    return out


def plan_of(case):
    """(regime, width, unaligned, head, accesses, tail, body wgs, edge wgs) for operands on
    a 16-B boundary plus the case's misalignments (sosx_block_copy_plan, host only)."""
    from sos_amd import shmem as S
    es, bsize, nblocks, dstr, sstr, dmis, smis = case
    out = (ctypes.c_longlong * 8)()
    assert S.lib().sosx_block_copy_plan((1 << 30) + dmis, dstr, (1 << 31) + smis, sstr, bsize, nblocks, es,
                                        out) == 0
    return tuple(out)


def thinned(es):
    """PER_SIZE cases of the sweep, chosen with a fixed seed, then topped up so that every
    regime the element size can reach, a head, a tail and the unaligned-load form are in."""
    full = sweep(es)
    rng = random.Random(0xB10C + es)
    picked = rng.sample(full, PER_SIZE)
    rng.shuffle(full)
    wants = [lambda p, r=r: p[0] == r for r in REGIMES]
    wants += [lambda p: p[0] == 4 and p[3] > 0, lambda p: p[0] == 4 and p[5] > 0,
              lambda p: p[0] == 5 and p[2] == 1, lambda p: p[0] == 5 and p[2] == 0 and p[5] > 0]
    for want in wants:
        if not any(want(plan_of(c)) for c in picked):
            extra = next((c for c in full if want(plan_of(c))), None)
            if extra:
                picked.append(extra)
    return picked


# one shape per regime whose grid has more than one workgroup (a tile is 1024 accesses)
MULTI_WG = [
    (4, 100, 300, 128, 256, 8, 8),    # congruent: head 8 B, 24 vectors, tail 8 B; 8 + 2 workgroups
    (4, 100, 300, 128, 101, 0, 4),    # incongruent, unaligned 16-B loads
    (4, 100, 300, 101, 128, 0, 0),    # incongruent, 4-B accesses on both sides
    (2, 40, 300, 64, 64, 2, 0),       # incongruent, 2-B accesses (below the unaligned form)
    (1, 1029, 257, 4099, 1030, 3, 5), # incongruent, single bytes
    (4, 3, 5000, 5, 7, 4, 12),        # small: 15000 elements
    (8, 1, 5000, 1, 3, 8, 0),         # single elements, target contiguous (pack)
    (2, 4, 3000, 8, 12, 0, 8),        # a small block that is one 8-B element
    (16, 5, 700, 6, 9, 0, 0),         # congruent by element size: 16-B elements
]


@pytest.fixture(scope="module")
def pool():
    """Random source bytes, generated once: every case reads a prefix of it."""
    n = 16 + 16 * 4099 * 257 // 4 + (1 << 16)
    return np.frombuffer(bytearray(np.random.default_rng(0xB10C).bytes(n)), dtype=np.uint8)


def run_case(torch, sos, pool, case):
    es, bsize, nblocks, dstr, sstr, dmis, smis = case
    bbytes = bsize * es
    sext = ((nblocks - 1) * sstr + bsize) * es
    dext = ((nblocks - 1) * dstr + bsize) * es
    assert smis + sext <= pool.size
    src_h = pool[:smis + sext]
    src_d = torch.from_numpy(src_h).cuda()
    total = GUARD + dmis + dext + GUARD
    dst_d = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    assert src_d.data_ptr() % 16 == 0 and dst_d.data_ptr() % 16 == 0
    sos.block_strided_copy(dst_d.data_ptr() + GUARD + dmis, dstr, src_d.data_ptr() + smis, sstr, bsize, nblocks, es)
    torch.cuda.synchronize()
    got = dst_d.cpu().numpy()
    exp = np.full(total, CANARY, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided
    view(exp[GUARD + dmis:], shape=(nblocks, bbytes), strides=(dstr * es, 1))[:] = \
        view(src_h[smis:], shape=(nblocks, bbytes), strides=(sstr * es, 1))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (f"es={es} bsize={bsize} nblocks={nblocks} dst_stride={dstr} src_stride={sstr} "
                           f"dmis={dmis} smis={smis} plan={plan_of(case)}: {bad.size} bytes differ, first at "
                           f"{bad[0] - GUARD - dmis} of the target extent {dext}")


@pytest.mark.parametrize("es", [1, 2, 4, 8, 16])
def test_block_copy_matches_numpy(torch_cuda, sos, pool, es):
    cases = thinned(es)
    assert PER_SIZE <= len(cases) <= PER_SIZE + 9
    seen = {plan_of(c)[0] for c in cases}
    # 16-B elements are always congruent or delegated; every other size reaches all five
    assert seen >= ({1, 4} if es == 16 else set(REGIMES)), seen
    for case in cases:
        run_case(torch_cuda, sos, pool, case)


@pytest.mark.parametrize("case", MULTI_WG, ids=lambda c: "es%d_b%d_n%d_d%d_s%d_%d_%d" % c)
def test_block_copy_more_than_one_workgroup(torch_cuda, sos, pool, case):
    p = plan_of(case)
    if p[0] >= 3:
        assert p[6] + p[7] > 1, p
    run_case(torch_cuda, sos, pool, case)


def test_multi_workgroup_cases_cover_the_regimes():
    plans = [plan_of(c) for c in MULTI_WG]
    assert {p[0] for p in plans} >= {2, 3, 4, 5}
    assert any(p[0] == 5 and p[2] == 1 for p in plans) and any(p[0] == 5 and p[1] == 1 for p in plans)
    assert any(p[0] == 4 and p[3] > 0 and p[5] > 0 for p in plans)
