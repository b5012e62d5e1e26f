"""CPU: the probe inputs of tests/fp_probes.py have teeth.

For every (type, op, P, order) fold and every prefix that tests/test_gpu_fold_specials.py
runs, with the oracle alone: exchanging any two inputs changes the reference (the plan
simulator's LINEAR / TREE fold, the in-order reduce_local prefix) in the vector body, in
the ragged tail and in the ragged head that the calls of the GPU test fold, under the
very comparison the GPU test applies.  A kernel that commutes one pair of inputs
therefore cannot pass there.

Two qualifications.  Long double: the x87 picks between two NaNs by significand and sign,
whatever side they are on, so only the min/max zero ties are required to show an exchange.
Complex prod: the GPU comparison takes any two NaNs as equal (which NaN a product carries
depends on gcc's register allocation on x86), and a complex product of finite values
commutes, so an exchange of inputs is required to show in the reference's bits only; the
elements compared as "NaN too" must stay under half of all elements.
"""
import numpy as np
import pytest

import fp_probes as F
import plansim

SEED = 29


def _differs(dt, op, ref, swapped):
    if dt in (F.CF, F.CD) and op == F.PROD:   # see the module docstring
        r, s = (x.view(np.uint8).reshape(x.size, -1) for x in (ref, swapped))
        return (r != s).any(axis=1)
    return ~F.elements_equal(dt, op, swapped, ref)


def _exchange_required(dt, op):
    return dt != F.LDBL or op in (F.MIN, F.MAX)


def _nan_share(dt, ref):
    ft = np.float32 if dt == F.CF else np.float64
    return float(np.isnan(ref.view(ft).reshape(-1, 2)).any(axis=1).mean())


def _check_exchanges(dt, op, P, ins, ref, fold, regions):
    """regions: {name: mask}; every exchange must show in every non-empty one."""
    if dt in (F.CF, F.CD) and op == F.PROD:
        assert _nan_share(dt, ref) <= 0.5
    if not _exchange_required(dt, op):
        return
    for j, k in F.all_pairs(P):
        sw = list(ins)
        sw[j], sw[k] = ins[k], ins[j]
        d = _differs(dt, op, ref, fold(sw))
        for name, mask in regions.items():
            if mask.any():
                assert d[mask].any(), f"exchange of inputs {j} and {k} does not show in the {name}"


def test_cycle_shape():
    for dt, op in F.FOLD_TYPES_OPS:
        for P in F.FOLD_P + F.RUNTIME_P:
            cyc = F.probe_kinds(dt, op, P)
            L = len(cyc)
            assert L % 2 == 1                                   # coprime to 64, 4, 2
            assert 3 * cyc.count(("ord",)) >= L
            assert L <= 1001                                    # the runtime-P tests' n
            named = {c[1:] for c in cyc if c[0] in (("tie", "tie_m") if op in (F.MIN, F.MAX) else ("nan2",))}
            if not (dt in (F.CF, F.CD) and op == F.PROD and P > F.FULL_P):  # thinned: its docstring
                assert set(F.all_pairs(P)) <= named
            if P <= 8:                                          # every kind in every pack lane
                vec = 16 // F.ELEM_SIZE[dt]
                assert F.big_n(dt) >= L * vec and F.prefix_big_n(dt) >= L * vec


def test_values_are_what_the_kinds_say():
    P, n = 5, 4000
    ins = F.probe_inputs(F.FLOAT, F.MIN, P, n, SEED)
    cyc = F.probe_kinds(F.FLOAT, F.MIN, P)
    bits = [a.view(np.uint32) for a in ins]
    seen = set()
    for i in range(n):
        kind = cyc[i % len(cyc)]
        col = [int(b[i]) for b in bits]
        if kind[0] == "nan2":
            j, k = kind[1:]
            assert np.isnan(ins[j][i]) and np.isnan(ins[k][i])
            assert col[j] & 0x3FFFFF == j + 1 and col[k] & 0x3FFFFF == k + 1
            assert (col[j] ^ col[k]) >> 31 == 1
            seen.add(("signalling", not (col[j] & col[k] & 0x400000)))
            assert all(np.isfinite(ins[p][i]) for p in range(P) if p not in (j, k))
        elif kind[0] in ("tie", "tie_m"):
            j, k = kind[1:]
            assert col[j] == (0x80000000 if kind[0] == "tie_m" else 0)
            assert col[k] == (0 if kind[0] == "tie_m" else 0x80000000)
            assert all(ins[p][i] > 1 for p in range(P) if p not in (j, k))
        elif kind[0] == "nan1":
            assert [p for p in range(P) if np.isnan(ins[p][i])] == [kind[1]]
        else:
            assert all(np.isfinite(ins[p][i]) for p in range(P))
    assert ("signalling", True) in seen and ("signalling", False) in seen
    ld = F.probe_inputs(F.LDBL, F.SUM, 3, 500, SEED)
    assert all((a.view(np.uint8).reshape(-1, 16)[:, 10:] != 0).all() for a in ld)
    cf = F.probe_inputs(F.CF, F.SUM, 3, 3000, SEED)
    parts = np.isnan(cf[0].view(np.float32).reshape(-1, 2))
    assert (parts[:, 0] & ~parts[:, 1]).any() and (~parts[:, 0] & parts[:, 1]).any() and parts.all(axis=1).any()


@pytest.mark.parametrize("order", [plansim.LINEAR, plansim.TREE])
@pytest.mark.parametrize("P", F.FOLD_P)
@pytest.mark.parametrize("dt,op", F.FOLD_TYPES_OPS)
def test_fold_exchanges_show(oracle, dt, op, P, order):
    es = F.ELEM_SIZE[dt]
    fold = lambda x: plansim.fold_values(op, dt, x, order)
    # k_fold_dyn, n = 1000: one call, no regions
    ins = F.probe_inputs(dt, op, P, 1000, SEED)
    _check_exchanges(dt, op, P, ins, fold(ins), fold, {"vector": np.ones(1000, bool)})
    # the vector kernels: every layout's regions over the windows the GPU test slides
    n = F.big_n(dt)
    total, starts = F.windows(dt, op, P, n)
    ins = F.probe_inputs(dt, op, P, total, SEED)
    ref = fold(ins)
    regions, heads, tails = {}, 0, 0
    for layout in F.FOLD_LAYOUTS:
        lo = F.layout_offsets(layout, es, P)
        if lo is None:
            continue
        for knobs in ((5, -1), (1, 0), (9, 1)):
            form, head, end = F.fold_form(es, P, n, lo[0], lo[1], *knobs)
            assert form != "k_fold_dyn(np<=8)"
            h, b, t = F.region_masks(total, starts, n, head, end)
            assert b.any()
            heads += h.any()
            tails += t.any()
            regions.update({f"head of {layout}/{form}": h, f"body of {layout}/{form}": b,
                            f"tail of {layout}/{form}": t})
    assert tails and (heads or es == 16)
    _check_exchanges(dt, op, P, ins, ref, fold, regions)


@pytest.mark.parametrize("order", [plansim.LINEAR, plansim.TREE])
@pytest.mark.parametrize("P", F.RUNTIME_P)
@pytest.mark.parametrize("dt,op", F.FOLD_TYPES_OPS)
def test_fold_runtime_p_exchanges_show(oracle, dt, op, P, order):
    fold = lambda x: plansim.fold_values(op, dt, x, order)
    ins = F.probe_inputs(dt, op, P, 1001, SEED)
    _check_exchanges(dt, op, P, ins, fold(ins), fold, {"vector": np.ones(1001, bool)})


@pytest.mark.parametrize("P", F.PREFIX_SUM_NP)
@pytest.mark.parametrize("dt", [F.FLOAT, F.DOUBLE, F.CF, F.CD, F.LDBL])
def test_prefix_sum_exchanges_show(oracle, dt, P):
    es, op = F.ELEM_SIZE[dt], F.SUM
    last = lambda x: F.cpu_prefix(op, dt, x)[-1]
    for n in (999, F.prefix_big_n(dt)):
        total, starts = F.windows(dt, op, P, n)
        ins = F.probe_inputs(dt, op, P, total, SEED)
        regions = {}
        for layout in F.PREFIX_LAYOUTS:
            lo = F.layout_offsets(layout, es, P)
            if lo is None:
                continue
            for knobs in ((5, -1), (1, 0), (9, 1)):
                form, head, end = F.prefix_form(es, op, P, n, lo[0], lo[1], *knobs)
                assert form != "k_prefix_dyn"
                h, b, t = F.region_masks(total, starts, n, head, end)
                regions.update({f"head of {layout}/{form}": h, f"body of {layout}/{form}": b,
                                f"tail of {layout}/{form}": t})
        _check_exchanges(dt, op, P, ins, last(ins), last, regions)


@pytest.mark.parametrize("P", F.PREFIX_DYN_NP)
@pytest.mark.parametrize("dt,op", F.PREFIX_DYN_TYPES_OPS)
def test_prefix_dyn_exchanges_show(oracle, dt, op, P):
    last = lambda x: F.cpu_prefix(op, dt, x)[-1]
    ins = F.probe_inputs(dt, op, P, 4099, SEED)
    _check_exchanges(dt, op, P, ins, last(ins), last, {"vector": np.ones(4099, bool)})
