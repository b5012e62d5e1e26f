"""GPU: the fold and prefix kernels on operand-order-sensitive fp values.

Inputs from tests/fp_probes.py: NaN pairs with a payload per input, +-0 ties, lone NaNs,
inf - inf and 0 * inf, the x87 cases for long double, laid in a cycle over oracle.fill
data so that every kind reaches every pack lane, the ragged head, the tile bodies and the
ragged tail (tests/test_fp_probes.py shows on the CPU that exchanging any two inputs
changes the expected bits in each of those regions).

  sosx_fold, both orders   == the plan simulator's LINEAR / TREE fold
  sosx_prefix              == the in-order prefix of the oracle's reduce_local
  loopback ring / recdbl   == oracle ring / recdbl, per PE
  loopback inscan / exscan == oracle scan

Bit for bit (all 16 bytes of a long double); complex prod by NaN equivalence
(test_gpu_combine.py::same_bits_nan_equiv).  The vector kernels are called on a window
[s, s + n) of the uploaded arrays, s advancing 16 bytes per call through one cycle of
probe kinds: every kind so takes the window's first and last elements in turn, which the
kernels fold in their element loops.  The windows are compared on the device; a failing
one is fetched and its first bad element named with its probe kind.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from sos_amd import _lib, shmem as S

import fp_probes as F
import plansim

pytestmark = pytest.mark.gpu

SEED = 29
GUARD = 0xA5


def upload(torch, a, off=0):
    """The bytes of `a`, `off` bytes past a 16-byte boundary of a fresh device buffer."""
    raw = np.frombuffer(a.tobytes(), np.uint8)
    t = torch.zeros(raw.size + off + 32, dtype=torch.uint8, device="cuda")
    t[off:off + raw.size].copy_(torch.from_numpy(raw.copy()))
    return t


def fetch(t, off, like):
    raw = t[off:off + like.nbytes].cpu().numpy()
    return np.frombuffer(raw.tobytes(), like.dtype).copy()


def device_mismatch(torch, dt, op, out, off, nbytes, exp):
    """0-d bool tensor: the result bytes differ from `exp` under the rule of (dt, op), or
    a byte around them was written."""
    got = out[off:off + nbytes]
    if dt in (F.CF, F.CD) and op == F.PROD:
        ft, it = (torch.float32, torch.int32) if dt == F.CF else (torch.float64, torch.int64)
        g, e = got.view(ft), exp.view(ft)
        bad = ~((g.view(it) == e.view(it)) | (g.isnan() & e.isnan())).all()
    else:
        bad = (got != exp).any()
    return bad | (out[:off] != GUARD).any() | (out[off + nbytes:] != GUARD).any()


def explain(dt, op, P, got, ref, start):
    ok = F.elements_equal(dt, op, got, ref)
    if ok.all():
        return "bytes around the result were written"
    i = int(np.nonzero(~ok)[0][0])
    return "%d bad elements; first at %s (window start %d, offset %d): got %s, expected %s" % (
        (~ok).sum(), F.describe(dt, op, P, start + i), start, i,
        got[i:i + 1].tobytes().hex(), ref[i:i + 1].tobytes().hex())


def slide(torch, dt, op, P, n, starts, refs, out_off, call):
    """Run call(out pointers, start) for every window start and compare output k with
    refs[k][start:start + n] on the device; one synchronisation for all windows."""
    es = F.ELEM_SIZE[dt]
    nb = n * es
    rdev = [upload(torch, r) for r in refs]
    outs = [torch.empty(nb + out_off + 48, dtype=torch.uint8, device="cuda") for _ in refs]
    flags = []

    def one(s):
        for o in outs:
            o.fill_(GUARD)
        call([o.data_ptr() + out_off for o in outs], s)

    for s in starts:
        one(s)
        for o, r in zip(outs, rdev):
            flags.append(device_mismatch(torch, dt, op, o, out_off, nb, r[s * es:s * es + nb]))
    bad = torch.stack(flags).cpu().numpy().reshape(len(starts), len(refs))
    if bad.any():
        w, k = (int(x) for x in np.argwhere(bad)[0])
        one(starts[w])
        torch.cuda.synchronize()
        got = fetch(outs[k], out_off, refs[k][:n])
        pytest.fail("output %d: %s" % (k, explain(dt, op, P, got, refs[k][starts[w]:starts[w] + n], starts[w])))


def run_fold(torch, dt, op, P, order, n, layout, slid):
    es = F.ELEM_SIZE[dt]
    out_off, in_offs = F.layout_offsets(layout, es, P)
    total, starts = F.windows(dt, op, P, n) if slid else (n, [0])
    ins = F.probe_inputs(dt, op, P, total, SEED)
    ref = plansim.fold_values(op, dt, ins, order)
    di = [upload(torch, a, off) for a, off in zip(ins, in_offs)]

    def call(outs, s):
        _lib.fold(op, dt, order, outs[0], [t.data_ptr() + off + s * es for t, off in zip(di, in_offs)], n)

    slide(torch, dt, op, P, n, starts, [ref], out_off, call)


def run_prefix(torch, dt, op, P, n, layout, slid):
    es = F.ELEM_SIZE[dt]
    out_off, in_offs = F.layout_offsets(layout, es, P)
    total, starts = F.windows(dt, op, P, n) if slid else (n, [0])
    ins = F.probe_inputs(dt, op, P, total, SEED)
    refs = F.cpu_prefix(op, dt, ins)
    di = [upload(torch, a, off) for a, off in zip(ins, in_offs)]

    def call(outs, s):
        _lib.prefix(op, dt, outs, [t.data_ptr() + off + s * es for t, off in zip(di, in_offs)], n)

    slide(torch, dt, op, P, n, starts, refs, out_off, call)


def _with_layout(types_ops, layouts):
    return [(dt, op, lay) for dt, op in types_ops for lay in layouts
            if F.layout_offsets(lay, F.ELEM_SIZE[dt], 2) is not None]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P", F.FOLD_P)
@pytest.mark.parametrize("dt,op,layout", _with_layout(F.FOLD_TYPES_OPS, ["grid", "past"]))
def test_fold_small_probes(torch_cuda, dt, op, layout, P, order):
    """k_fold_dyn, at most 8 inputs of n = 1000 elements, on and off a 16-byte boundary."""
    assert F.fold_form(F.ELEM_SIZE[dt], P, 1000, *F.layout_offsets(layout, F.ELEM_SIZE[dt], P))[0] \
        == "k_fold_dyn(np<=8)"
    run_fold(torch_cuda, dt, op, P, order, 1000, layout, slid=False)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P", F.FOLD_P)
@pytest.mark.parametrize("dt,op,layout", _with_layout(F.FOLD_TYPES_OPS, ["grid", "past"]))
def test_fold_vector_probes(torch_cuda, dt, op, layout, P, order):
    """k_fold: everything congruent, the output on the 16-byte grid (a ragged tail) and
    one element past it (a ragged head too)."""
    n = F.big_n(dt)
    assert F.fold_form(F.ELEM_SIZE[dt], P, n, *F.layout_offsets(layout, F.ELEM_SIZE[dt], P))[0] == "k_fold"
    run_fold(torch_cuda, dt, op, P, order, n, layout, slid=True)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P", F.FOLD_P)
@pytest.mark.parametrize("dt,op,layout", _with_layout(F.FOLD_TYPES_OPS, ["own", "mixed", "peers_es"]))
def test_fold_realigned_probes(torch_cuda, dt, op, layout, P, order):
    """Inputs at other 16-byte offsets than the output: k_fold_realign_np by DPP ("own";
    "mixed" with fewer than five inputs off the grid) or by unaligned loads ("mixed" with
    five or more, "peers_es"); test_forms_forced reruns these under the other forms,
    k_fold_outshift among them."""
    n = F.big_n(dt)
    form = F.fold_form(F.ELEM_SIZE[dt], P, n, *F.layout_offsets(layout, F.ELEM_SIZE[dt], P))[0]
    assert form.startswith("k_fold_realign_np")
    run_fold(torch_cuda, dt, op, P, order, n, layout, slid=True)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P", F.RUNTIME_P)
@pytest.mark.parametrize("dt,op", F.FOLD_TYPES_OPS)
def test_fold_runtime_p_probes(torch_cuda, dt, op, P, order):
    """k_fold_dyn above 8 inputs: the LINEAR loop and the TREE stack walk."""
    run_fold(torch_cuda, dt, op, P, order, 1001, "grid", slid=False)


@pytest.mark.parametrize("P", F.PREFIX_SUM_NP)
@pytest.mark.parametrize("dt,layout", [(dt, lay) for dt, _, lay in
                                       _with_layout([(d, F.SUM) for d in (F.FLOAT, F.DOUBLE, F.CF, F.CD, F.LDBL)],
                                                    ["grid", "past"])])
def test_prefix_vector_probes(torch_cuda, dt, layout, P):
    """k_prefix: sum, inputs and outputs congruent."""
    for n in (999, F.prefix_big_n(dt)):
        assert F.prefix_form(F.ELEM_SIZE[dt], F.SUM, P, n, *F.layout_offsets(layout, F.ELEM_SIZE[dt], P))[0] \
            == "k_prefix"
        run_prefix(torch_cuda, dt, F.SUM, P, n, layout, slid=True)


@pytest.mark.parametrize("P", F.PREFIX_SUM_NP)
@pytest.mark.parametrize("dt,layout", [(dt, lay) for dt, _, lay in
                                       _with_layout([(d, F.SUM) for d in (F.FLOAT, F.DOUBLE, F.CF)],
                                                    ["first", "each", "all"])])
def test_prefix_realigned_probes(torch_cuda, dt, layout, P):
    """Sum prefix with inputs at other 16-byte offsets than the outputs: input 0 only,
    each input at its own offset, all at one (k_prefix_realign_np by DPP or unaligned
    loads, k_prefix_outshift; test_forms_forced reruns these under the other forms)."""
    for n in (999, F.prefix_big_n(dt)):
        form = F.prefix_form(F.ELEM_SIZE[dt], F.SUM, P, n, *F.layout_offsets(layout, F.ELEM_SIZE[dt], P))[0]
        assert form in ("k_prefix_realign_np(DPP)", "k_prefix_realign_np(unaligned loads)", "k_prefix_outshift")
        run_prefix(torch_cuda, dt, F.SUM, P, n, layout, slid=True)


@pytest.mark.parametrize("P", F.PREFIX_DYN_NP)
@pytest.mark.parametrize("dt,op", F.PREFIX_DYN_TYPES_OPS)
def test_prefix_dyn_probes(torch_cuda, dt, op, P):
    """min, max and prod through k_prefix_dyn, out of place and as the in-place exscan of
    test_prefix_kernel_aliasing (output j-1 is input j's buffer; `own` above 8 inputs)."""
    torch = torch_cuda
    n = 4099
    assert F.prefix_form(F.ELEM_SIZE[dt], op, P, n, 0, [0] * P)[0] == "k_prefix_dyn"
    run_prefix(torch, dt, op, P, n, "grid", slid=False)
    ins = F.probe_inputs(dt, op, P, n, SEED)
    refs = F.cpu_prefix(op, dt, ins)
    j = P // 2
    di = [upload(torch, a) for a in ins]
    do = [torch.zeros_like(t) for t in di]
    do[j - 1] = di[j]
    _lib.prefix(op, dt, [t.data_ptr() for t in do], [t.data_ptr() for t in di], n, own=j if P > 8 else -1)
    torch.cuda.synchronize()
    for k in range(P):
        got = fetch(do[k], 0, refs[k])
        assert F.elements_equal(dt, op, got, refs[k]).all(), \
            "in place, output %d: %s" % (k, explain(dt, op, P, got, refs[k], 0))


@pytest.mark.parametrize("form", ["unaligned", "shifted"])
def test_forms_forced(form):
    """The realigned cases above under every form of the realigning kernels, each in a
    child process (the switches are read once per process).  "unaligned": every layout
    with an incongruent input loads unaligned; "shifted": the register-realigned forms
    only (DPP per input; k_fold_outshift and k_prefix_outshift for one-offset layouts)."""
    here = os.path.abspath(__file__)
    knobs = {"unaligned": ("1", "0"), "shifted": ("9", "1")}[form]
    env = dict(os.environ, SOSX_REALIGN_UNALIGNED=knobs[0], SOSX_FOLD_OUTSHIFT=knobs[1],
               SOSX_PREFIX_OUTSHIFT=knobs[1])
    r = subprocess.run([sys.executable, "-m", "pytest", here, "-q", "-p", "no:cacheprovider", "-m", "gpu", "-k",
                        "test_fold_realigned_probes or test_prefix_realigned_probes"],
                       capture_output=True, text=True, timeout=280, env=env,
                       cwd=os.path.dirname(os.path.dirname(here)))
    assert r.returncode == 0, (r.stdout[-2500:], r.stderr[-1500:])
    assert " passed" in r.stdout and "failed" not in r.stdout


def _loopback(torch, alg, op, dt, srcs, in_place):
    ds = [upload(torch, a) for a in srcs]
    dd = ds if in_place else [torch.zeros_like(t) for t in ds]
    S.loopback_allreduce(alg, op, dt, [t.data_ptr() for t in ds], [t.data_ptr() for t in dd], srcs[0].size)
    torch.cuda.synchronize()
    return [fetch(dd[p], 0, srcs[p]) for p in range(len(srcs))]


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("dt,op", [(F.FLOAT, F.MIN), (F.DOUBLE, F.SUM)])
@pytest.mark.parametrize("alg", ["ring", "recdbl"])
def test_loopback_allreduce_probes(torch_cuda, alg, dt, op, P, in_place):
    """The executor's input permutation: every PE's result of the ring (each chunk past
    64 KiB) and of recursive doubling, against the oracle's per-PE values."""
    n = P * 65536 // F.ELEM_SIZE[dt] + 4099
    srcs = F.probe_inputs(dt, op, P, n, SEED)
    ref = (O.ring if alg == "ring" else O.recdbl)(op, dt, [a.copy() for a in srcs])
    got = _loopback(torch_cuda, alg, op, dt, srcs, in_place)
    for p in range(P):
        assert F.elements_equal(dt, op, got[p], ref[p]).all(), \
            "PE %d: %s" % (p, explain(dt, op, P, got[p], ref[p], 0))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("P", [3, 8])
def test_loopback_scan_probes(torch_cuda, P, exclusive, in_place):
    dt, op, n = F.FLOAT, F.SUM, 4096 + 3
    srcs = F.probe_inputs(dt, op, P, n, SEED)
    ref = O.scan(op, dt, [a.copy() for a in srcs], exclusive)
    got = _loopback(torch_cuda, _lib.PLAN_EXSCAN if exclusive else _lib.PLAN_INSCAN, op, dt, srcs, in_place)
    for p in range(P):
        assert F.elements_equal(dt, op, got[p], ref[p]).all(), \
            "PE %d: %s" % (p, explain(dt, op, P, got[p], ref[p], 0))
