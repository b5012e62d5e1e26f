"""Directed x87 80-bit encodings for the long double GPU tests (test infrastructure).

A subset of the list tests/ldbl_x87_harness.cpp runs on the host, as raw bytes: numpy
never does arithmetic on these values (signalling NaNs and unsupported encodings would
not survive it), arrays are built and permuted as (n, 16) uint8 and only viewed as
np.longdouble for the oracle.
"""
import numpy as np

BIAS = 16383

EXPONENTS = [0, 1, 2, 64, 128, BIAS - 65, BIAS - 64, BIAS - 63, BIAS - 1, BIAS, BIAS + 1,
             0x403E, 0x403F, 0x4040, 0x1FFF, 0x2000, 0x5FFF, 0x6000, 0x7FFD, 0x7FFE, 0x7FFF]

SIGNIFICANDS = [
    # integer bit clear: zero, denormals; unnormals, pseudo-infinity and pseudo-NaNs
    0x0000000000000000, 0x0000000000000001, 0x0000000000000003, 0x4000000000000000,
    0x7FFFFFFFFFFFFFFF,
    # integer bit set: normals, pseudo-denormals, infinity, signalling NaNs
    0x8000000000000000, 0x8000000000000001, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE,
    # exact rounding ties of products and sums
    0x8000000080000000, 0xC000000080000000, 0xFFFFFFFF80000000, 0xAAAAAAAAAAAAAAAA,
    0xD555555555555555,
    # NaN payloads, quiet and signalling, pairs that differ in bit 62 only
    0xC000000000000000, 0xC000000000000001, 0xC000000000000123, 0x8000000000000123,
    0xBFFFFFFFFFFFFFFF, 0xA000000000000000,
]

PAD_A = bytes([0xF6, 0xE5, 0xD4, 0xC3, 0xB2, 0xA1])
PAD_B = bytes([0x5C, 0x4B, 0x3A, 0x29, 0x18, 0x07])


def encode(sign, exp, m, pad=bytes(6)):
    """The 16 bytes of one long double: significand, sign | exponent, 6 padding bytes."""
    return m.to_bytes(8, "little") + ((sign << 15) | exp).to_bytes(2, "little") + bytes(pad)


def encodings():
    """(840, 16) uint8: every sign x exponent field x significand, padding zero."""
    rows = [encode(s, e, m) for e in EXPONENTS for m in SIGNIFICANDS for s in (0, 1)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 16).copy()


def padded(raw, pad):
    """Copy of the (n, 16) byte rows with the 6 padding bytes set to `pad`."""
    out = raw.copy()
    out[:, 10:] = np.frombuffer(bytes(pad), np.uint8)
    return out


def as_ld(raw):
    """The rows as an np.longdouble array (a copy; no conversion)."""
    return np.ascontiguousarray(raw).reshape(-1).view(np.longdouble).copy()


def all_pairs():
    """(a, b): every ordered pair of the encodings, `a` and `b` with different padding."""
    v = encodings()
    n = len(v)
    ia, ib = np.divmod(np.arange(n * n), n)
    return as_ld(padded(v, PAD_A)[ia]), as_ld(padded(v, PAD_B)[ib])


def permuted_inputs(P, n, seed):
    """P arrays of n long doubles: input k is the encoding list (tiled to n, every fourth
    place a NaN so that a few percent of the elements meet two of them) under the seeded
    permutation k, with padding bytes of its own, so at every index each input holds
    another NaN payload, sign or encoding."""
    v = encodings()
    base = v[np.arange(n) % len(v)]
    nans = np.frombuffer(b"".join(encode(s, 0x7FFF, m) for m in SIGNIFICANDS for s in (0, 1)
                                  if m >> 63 and m << 1 & (1 << 64) - 1), np.uint8).reshape(-1, 16)
    base[3::4] = nans[np.arange(len(base[3::4])) % len(nans)]
    ins = []
    for k in range(P):
        perm = np.random.default_rng(seed * 1000 + k).permutation(n)
        ins.append(as_ld(padded(base[perm], bytes([0x11 * (k % 15 + 1)] * 5 + [k + 1]))))
    return ins


def bad_rows(got, ref):
    """Indices of the elements whose 16 bytes differ."""
    g = got.view(np.uint8).reshape(-1, 16)
    r = ref.view(np.uint8).reshape(-1, 16)
    return np.nonzero((g != r).any(axis=1))[0]


def show(arr, i):
    row = arr.view(np.uint8).reshape(-1, 16)[i]
    return f"{int.from_bytes(bytes(row[8:10]), 'little'):04x}:{int.from_bytes(bytes(row[:8]), 'little'):016x}" \
           f"|{bytes(row[10:][::-1]).hex()}"
