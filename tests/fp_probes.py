"""Operand-order-sensitive fp inputs for the fold and prefix kernels (test infrastructure).

probe_inputs(dt, op, P, n, seed) lays a fixed cycle of *probe kinds* over ordinary
oracle.fill data.  A kind fixes what every one of the P inputs holds at that element, so
a kernel that commutes one pair of inputs, or walks the recdbl_sw tree with the wrong
side as "own", yields another NaN payload or another zero sign there:

  ("nan2", j, k)   inputs j and k hold NaNs with payloads j+1 and k+1 and opposite signs
                   (four variants: which one is negative, and one of them signalling);
  ("tie", j, k)    +0 at j, -0 at k, every other input a value that cannot win (min/max);
  ("tie_m", j, k)  the mirrored tie;
  ("nan1", k)      a lone NaN at input k (min/max);
  ("inv", j, k)    inf - inf (sum) or 0 * inf (prod) at (j, k): the default NaN, with a
                   payload NaN at input k + 1 where there is one;
  ("ld_qs",), ("ld_eqsig",), ("ld_zeros",)   long double only: every input a NaN, quiet
                   on the even inputs and signalling with a larger payload on the odd ones;
                   one significand on every input with mixed signs; zeros of mixed sign;
  ("ord",)         an ordinary element.

The variant of a kind (NaN signs and the signalling one, the complex part that carries
the probe: real, imaginary, both) rotates with the cycle's repetition, so every variant
of every kind comes round.  The cycle length is odd: coprime to 64 and to the pack
widths 1, 2 and 4, so a kind lands in every lane of a 16-byte pack, and the GPU tests
slide their window over the arrays one cycle slot at a time, which brings every kind into
the ragged head and the ragged tail.  At least a third of the slots are ordinary.

Teams above FULL_P inputs (the runtime-P kernels at n = 1001) take a thinned cycle that
still holds every pair once in the family its op is sensitive to: NaN pairs for sum and
prod, zero ties (the orientation rotating) for min and max; the other pair families keep
the adjacent pairs only.  Complex prod keeps two ordinary elements per probe, and above
FULL_P only the NaN pairs at most ten inputs apart and the tree's extras with their
partners: its NaN results can only be compared as "NaN too", and such elements stay under
half of every vector.

The module also restates the host dispatch of sosx_fold and sosx_prefix (fold_form,
prefix_form, geometry), so that the tests know which elements a call folds in its ragged
head, its vector body and its ragged tail, and which kernel form a layout reaches.
"""
import numpy as np

from oracle import oracle as O

import ldbl_vectors as V

FLOAT, DOUBLE, LDBL, CF, CD = 23, 24, 25, 26, 27
MIN, MAX, SUM, PROD = 3, 4, 5, 6
OP_NAMES = {MIN: "min", MAX: "max", SUM: "sum", PROD: "prod"}
FULL_P = 12
PARTS = ("re", "im", "re+im")

ELEM_SIZE = {FLOAT: 4, DOUBLE: 8, LDBL: 16, CF: 8, CD: 16}


def all_pairs(P):
    return [(j, k) for j in range(P) for k in range(j + 1, P)]


def probe_kinds(dt, op, P):
    """The cycle of probe kinds for P inputs of type dt under op (a list of tuples)."""
    minmax = op in (MIN, MAX)
    assert not (minmax and dt in (CF, CD))
    full = P <= FULL_P
    pairs = all_pairs(P)
    adjacent = [(j, j + 1) for j in range(P - 1)]
    thin_prod = dt in (CF, CD) and op == PROD and not full
    if thin_prod:
        # complex prod compares a NaN part as "NaN too", and those elements must stay under
        # half of n = 1001: the pairs at most ten inputs apart, and the tree's extras with
        # their partners (a finite complex product commutes, so only a NaN pair shows those)
        p2 = 1 << (P.bit_length() - 1)
        probes = [("nan2", j, k) for j, k in pairs if k - j <= 10 or k - j == p2]
    else:
        probes = [("nan2", j, k) for j, k in (pairs if full or not minmax else adjacent)]
    if minmax:
        probes += [("tie", j, k) for j, k in pairs]
        if full:
            probes += [("tie_m", j, k) for j, k in pairs]
        probes += [("nan1", k) for k in range(P)]
    else:
        probes += [("inv", j, k) for j, k in (pairs if full else adjacent)]
    if dt == LDBL:
        probes += [("ld_qs",), ("ld_eqsig",), ("ld_zeros",)]
    # complex prod: a probe mostly leaves a NaN part, which the device comparison can only
    # check as "NaN too": two ordinary elements per probe keep those under half
    per = 1 if (dt in (CF, CD) and op == PROD) else 2
    cycle = []
    for i, k in enumerate(probes):
        cycle.append(k)
        if i % per == per - 1:
            cycle += [("ord",)] * (1 if per == 2 else 2)
    while len(cycle) % 2 == 0 or 3 * cycle.count(("ord",)) < len(cycle):
        cycle.append(("ord",))
    return cycle


def describe(dt, op, P, i):
    """The probe kind (and its variant) at element i, for assert messages."""
    cyc = probe_kinds(dt, op, P)
    L = len(cyc)
    kind, rot = cyc[i % L], i // L + i % L
    s = "%s%s" % (kind[0], tuple(kind[1:]) if len(kind) > 1 else "")
    if kind[0] in ("nan2", "inv", "nan1", "tie"):
        s += " v%d" % (rot % 4)
    if dt in (CF, CD) and kind[0] != "ord":
        s += " " + PARTS[(rot // 4) % 3]
    return "element %d: %s" % (i, s)


class _Bits:
    """Writes special values into input arrays of one type, by bit pattern."""

    def __init__(self, dt, srcs):
        self.dt = dt
        self.srcs = srcs
        if dt == LDBL:
            self.rows = [a.view(np.uint8).reshape(-1, 16) for a in srcs]
        else:
            self.ity = np.uint32 if dt in (FLOAT, CF) else np.uint64
            c = 2 if dt in (CF, CD) else 1
            self.u = [a.view(self.ity).reshape(-1, c) for a in srcs]
            self.f = [a.view(np.float32 if dt in (FLOAT, CF) else np.float64).reshape(-1, c) for a in srcs]

    def cols(self, part):
        if self.dt not in (CF, CD):
            return [0]
        return [[0], [1], [0, 1]][part]

    def _enc(self, what, sign, payload=0, signalling=False):
        if self.dt == LDBL:
            if what == "nan":
                m = (0x8000000000000100 if signalling else 0xC000000000000000) | payload
                return np.frombuffer(V.encode(sign, 0x7FFF, m)[:10], np.uint8)
            if what == "inf":
                return np.frombuffer(V.encode(sign, 0x7FFF, 0x8000000000000000)[:10], np.uint8)
            return np.frombuffer(V.encode(sign, 0, 0)[:10], np.uint8)
        if self.ity == np.uint32:
            sb, ex, q = 31, 0x7F800000, 0x00400000
        else:
            sb, ex, q = 63, 0x7FF0000000000000, 0x0008000000000000
        if what == "nan":
            return self.ity((sign << sb) | ex | (0 if signalling else q) | payload)
        if what == "inf":
            return self.ity((sign << sb) | ex)
        return self.ity(sign << sb)

    def put(self, p, idx, part, what, sign, payload=0, signalling=False):
        v = self._enc(what, int(sign), payload, signalling)
        if self.dt == LDBL:
            self.rows[p][idx, :10] = v
        else:
            for c in self.cols(part):
                self.u[p][idx, c] = v

    def cannot_win(self, p, idx, op):
        """|x| + 1.5 for min, its negative for max: loses against either zero."""
        s = 1 if op == MIN else -1
        if self.dt == LDBL:
            self.srcs[p][idx] = s * (np.abs(self.srcs[p][idx]) + np.longdouble(1.5))
        else:
            self.f[p][idx, 0] = s * (np.abs(self.f[p][idx, 0]) + 1.5)


def ordinary(dt, op, p, n, seed):
    if dt == LDBL:
        return np.random.default_rng(seed * 131 + p).standard_normal(n).astype(np.longdouble)
    return O.fill(dt, 1 if op == PROD else 0, seed, p, n)


def probe_inputs(dt, op, P, n, seed):
    """P arrays of n elements: oracle.fill data under the probe cycle of (dt, op, P)."""
    srcs = [ordinary(dt, op, p, n, seed) for p in range(P)]
    B = _Bits(dt, srcs)
    cyc = probe_kinds(dt, op, P)
    L = len(cyc)
    cplx = dt in (CF, CD)
    for slot, kind in enumerate(cyc):
        if kind[0] == "ord" or slot >= n:
            continue
        at = np.arange(slot, n, L)
        rot = at // L + slot
        for v in range(4):
            for part in range(3 if cplx else 1):
                idx = at[(rot % 4 == v) & (((rot // 4) % 3 == part) if cplx else True)]
                if idx.size:
                    _lay(B, kind, idx, v, part, op, P)
    if dt == LDBL:
        rng = np.random.default_rng(seed + 77)
        for p in range(P):
            B.rows[p][:, 10:] = rng.integers(1, 256, (n, 6), dtype=np.uint8)
    return srcs


def _lay(B, kind, idx, v, part, op, P):
    name = kind[0]
    if name == "nan2":
        j, k = kind[1], kind[2]
        # v0 (+q, -q)  v1 (-q, +q)  v2 (+s, -q)  v3 (-q, +s)
        B.put(j, idx, part, "nan", v in (1, 3), j + 1, signalling=v == 2)
        B.put(k, idx, part, "nan", v in (0, 2), k + 1, signalling=v == 3)
    elif name in ("tie", "tie_m"):
        j, k = kind[1], kind[2]
        # above FULL_P there is no mirrored kind: the orientation rotates instead
        neg_j = (name == "tie_m") or (P > FULL_P and v % 2 == 1)
        for p in range(P):
            if p == j:
                B.put(p, idx, part, "zero", neg_j)
            elif p == k:
                B.put(p, idx, part, "zero", not neg_j)
            else:
                B.cannot_win(p, idx, op)
    elif name == "nan1":
        B.put(kind[1], idx, part, "nan", v % 2, kind[1] + 1, signalling=v >= 2)
    elif name == "inv":
        j, k = kind[1], kind[2]
        a, b = (j, k) if v % 2 == 0 else (k, j)
        if op == SUM:
            B.put(a, idx, part, "inf", 0)
            B.put(b, idx, part, "inf", 1)
        else:
            B.put(a, idx, part, "zero", v >= 2)
            B.put(b, idx, part, "inf", v == 1)
        if k + 1 < P:
            B.put(k + 1, idx, part, "nan", v >= 2, k + 2)
    elif name == "ld_qs":
        for p in range(P):
            B.put(p, idx, part, "nan", p % 3 == 2, p + 1, signalling=p % 2 == 1)
    elif name == "ld_eqsig":
        for p in range(P):
            B.put(p, idx, part, "nan", (p + 1) % 2, 7)
    elif name == "ld_zeros":
        for p in range(P):
            B.put(p, idx, part, "zero", p % 2)


# -----------------------------------------------------------------------------------
# The host dispatch of sosx_fold / sosx_prefix restated (fold_order.hip, fold.hip,
# elementwise.h make_geom): which kernel form a layout reaches, and its regions.
# -----------------------------------------------------------------------------------
K_THREADS = 256
SPREAD_BYTES = 64 * 1024


def geometry(addr_mod16, n, es, U):
    """(head, body_end): elements [0, head) and [body_end, n) go through the element
    loops of the remainder workgroup, [head, body_end) through 16-byte vectors."""
    mis = addr_mod16 & 15
    head = min((16 - mis) // es if mis else 0, n)
    vec = 16 // es
    tiles = ((n - head) // vec) // (K_THREADS * U)
    return head, head + tiles * K_THREADS * U * vec


def fold_form(es, P, n, out_mod, in_mods, unaligned_min=5, outshift=-1):
    """(kernel form, head, body_end) of sosx_fold over P inputs at the given addresses
    mod 16; the two knobs are SOSX_REALIGN_UNALIGNED and SOSX_FOLD_OUTSHIFT."""
    if P > 8:
        return "k_fold_dyn(runtime P)", 0, 0
    congruent = out_mod % es == 0 and es <= 16 and all((m ^ out_mod) & 15 == 0 for m in in_mods)
    elem_aligned = out_mod % es == 0 and all(m % es == 0 for m in in_mods)
    if es < 16 and not congruent and elem_aligned and n * es > SPREAD_BYTES:
        head, end = geometry(out_mod, n, es, 1)
        d = [(m + head * es) & 15 for m in in_mods]
        one_offset = all(x == d[0] for x in d) and d[0] != 0
        m = sum(x != 0 for x in d)
        ul_ok = es in (4, 8)
        if one_offset and (outshift > 0 or (outshift < 0 and not ul_ok)):
            return "k_fold_outshift", head, end
        if ul_ok and (m >= unaligned_min or (one_offset and outshift < 0)):
            return "k_fold_realign_np(unaligned loads)", head, end
        return "k_fold_realign_np(DPP)", head, end
    if not congruent or n * es <= SPREAD_BYTES:
        return "k_fold_dyn(np<=8)", 0, 0
    U = 4 if P <= 2 else 2 if P <= 4 else 1
    head, end = geometry(out_mod, n, es, U)
    return "k_fold", head, end


def prefix_form(es, op, P, n, out_mod, in_mods, unaligned_min=5, outshift=-1):
    """As fold_form, for sosx_prefix with every output at out_mod."""
    congruent = out_mod % es == 0 and all((m ^ out_mod) & 15 == 0 for m in in_mods)
    if op == SUM and P <= 8:
        if not congruent and out_mod % es == 0 and all(m % es == 0 for m in in_mods):
            head, end = geometry(out_mod, n, es, 1)
            d = [(m + head * es) & 15 for m in in_mods]
            one_offset = all(x == d[0] for x in d) and d[0] != 0
            m = sum(x != 0 for x in d)
            ul_ok = es in (4, 8)
            ul_one = ul_ok and (P == 1 or P >= 5)
            shift = one_offset and (outshift > 0 or (outshift < 0 and not ul_one))
            if shift:
                return "k_prefix_outshift", head, end
            if ul_ok and (m >= unaligned_min or (one_offset and outshift < 0)):
                return "k_prefix_realign_np(unaligned loads)", head, end
            return "k_prefix_realign_np(DPP)", head, end
        if congruent:
            head, end = geometry(out_mod, n, es, 1)
            return "k_prefix", head, end
    return "k_prefix_dyn", 0, 0


# -----------------------------------------------------------------------------------
# The cases of tests/test_gpu_fold_specials.py, shared with tests/test_fp_probes.py (which
# checks on the CPU that an exchanged pair of inputs shows in every region they reach).
# -----------------------------------------------------------------------------------
FOLD_TYPES_OPS = ([(dt, op) for dt in (FLOAT, DOUBLE) for op in (MIN, MAX, SUM, PROD)]
                  + [(dt, op) for dt in (CF, CD) for op in (SUM, PROD)]
                  + [(LDBL, op) for op in (MIN, MAX, SUM, PROD)])
FOLD_P = [2, 3, 5, 7, 8]
RUNTIME_P = [9, 12, 33]
PREFIX_SUM_NP = [2, 3, 5, 8]
PREFIX_DYN_NP = [3, 8, 12]
PREFIX_DYN_TYPES_OPS = ([(dt, op) for dt in (FLOAT, DOUBLE, LDBL) for op in (MIN, MAX, PROD)]
                        + [(CF, PROD), (CD, PROD)])
FOLD_LAYOUTS = ["grid", "past", "own", "mixed", "peers_es"]
PREFIX_LAYOUTS = ["grid", "past", "first", "each", "all"]


def big_n(dt):
    """Past the 64 KiB below which sosx_fold spreads one element per lane."""
    return 65536 // ELEM_SIZE[dt] + 4099


def prefix_big_n(dt):
    return 16384 // ELEM_SIZE[dt] + 4099


def layout_offsets(layout, es, P):
    """(output offset, input offsets) in bytes past a 16-byte boundary; None when the
    layout does not exist for this element size (16-byte elements are always congruent)."""
    if layout == "grid":
        return 0, [0] * P
    if es >= 16:
        return None
    if layout == "past":                      # everything one element past the grid
        return es, [es] * P
    if layout in ("own", "first"):            # input 0 only
        return 0, [es] + [0] * (P - 1)
    if layout == "mixed":
        return 0, [(es * k) % 16 for k in range(1, P + 1)]
    if layout == "each":
        return 0, [(es * (k + 1)) % 16 for k in range(P)]
    return 0, [es % 16] * P                   # "peers_es", "all"


def windows(dt, op, P, n):
    """(total elements, window starts): a call folds elements [s, s + n) of the arrays.
    One start per cycle slot, 16 bytes apart, so that the window's first and last elements
    (its ragged head and tail) take every slot of the cycle in turn."""
    vec = 16 // ELEM_SIZE[dt]
    L = len(probe_kinds(dt, op, P))
    starts = [vec * m for m in range(L)]
    return n + vec * L, starts


def region_masks(total, starts, n, head, body_end):
    """Boolean masks over the arrays' elements: in some window's ragged head, vector body,
    ragged tail."""
    h = np.zeros(total, bool)
    b = np.zeros(total, bool)
    t = np.zeros(total, bool)
    for s in starts:
        h[s:s + head] = True
        b[s + head:s + body_end] = True
        t[s + body_end:s + n] = True
    return h, b, t


def nan_equiv_equal(a, b):
    """Per element: bitwise equal, or both NaN in the same part (complex prod only)."""
    ft = np.float32 if a.dtype == np.complex64 else np.float64
    it = np.uint32 if ft == np.float32 else np.uint64
    x, y = a.view(ft).reshape(-1, 2), b.view(ft).reshape(-1, 2)
    ok = (x.view(it) == y.view(it)) | (np.isnan(x) & np.isnan(y))
    return ok.all(axis=1)


def elements_equal(dt, op, got, ref):
    """Per-element verdict under the comparison rule of (dt, op): bit for bit (all 16
    bytes of a long double), complex prod by NaN equivalence."""
    if dt in (CF, CD) and op == PROD:
        return nan_equiv_equal(got, ref)
    es = ELEM_SIZE[dt]
    g = np.frombuffer(got.tobytes(), np.uint8).reshape(-1, es)
    r = np.frombuffer(ref.tobytes(), np.uint8).reshape(-1, es)
    return (g == r).all(axis=1)


def cpu_prefix(op, dt, ins):
    acc = ins[0].copy()
    outs = [acc.copy()]
    for x in ins[1:]:
        O.reduce_local(op, dt, x, acc)
        outs.append(acc.copy())
    return outs
