"""Generate tests/golden/onesided_refusals.json: a frozen record of what the one-sided layer's
argument checks answer -- (function, layout, op, code, message) for a fixed grid of cases.

TEST INFRASTRUCTURE.  The five exported check functions (sos_rma_check, sos_amo_check,
sos_put_signal_check, sos_sync_check, sos_lock_check) are called through sos_amd.shmem over the
made-up layout of tests/test_lock_checks.py (a device heap DEV, a host heap HOSTH, a data
segment DATA_BASE, and LOCAL, an address in none of them).  tests/test_onesided_refusals.py
replays the file against the built library and requires the same code and the same message
bytes for every case, so a refactoring of the checks that moves one refusal, or one byte of
its text, fails on the CPU.

The file is a record of a COMMIT, not of the working tree: the script refuses to run when
sos_amd/csrc differs from HEAD, and writes HEAD's id into the file.  Regenerate it only from
the parent of a change that means to alter a refusal, never from the code under test.

Usage: python tests/golden/make_refusals.py   (rewrites onesided_refusals.json next to it)
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

HOST_HEAP, DEVICE_HEAP, DATA = 0, 1, 2
DEV, DEV_SIZE = 0x7F0000000000, 1 << 20
HOSTH, HOSTH_SIZE = 0x500000000000, 1 << 16
DATA_BASE, DATA_SIZE = 0x600000, 4096
LOCAL = 0x10000
REGIONS = [(DEV, DEV_SIZE, DEVICE_HEAP), (HOSTH, HOSTH_SIZE, HOST_HEAP), (DATA_BASE, DATA_SIZE, DATA)]
ME, OTHER, N_PES = 1, 2, 4
ONE, ALL, ANY, SOME = range(4)
MSG_LEN = 512
_c = ctypes


class Region(_c.Structure):
    _fields_ = [("base", _c.c_size_t), ("size", _c.c_size_t), ("kind", _c.c_int)]


class Layout(_c.Structure):
    _fields_ = [("initialized", _c.c_int), ("my_pe", _c.c_int), ("n_pes", _c.c_int), ("mapped", _c.c_int),
                ("nregions", _c.c_int), ("regions", _c.POINTER(Region))]


class RmaOp(_c.Structure):
    _fields_ = [("remote", _c.c_void_p), ("local", _c.c_void_p), ("remote_stride", _c.c_ssize_t),
                ("local_stride", _c.c_ssize_t), ("bsize", _c.c_size_t), ("nblocks", _c.c_size_t),
                ("type_size", _c.c_size_t), ("pe", _c.c_int), ("put", _c.c_int), ("strided", _c.c_int)]


class AmoOp(_c.Structure):
    _fields_ = [("target", _c.c_void_p), ("fetch", _c.c_void_p), ("type_size", _c.c_size_t), ("pe", _c.c_int),
                ("nbi", _c.c_int)]


class PutSignalOp(_c.Structure):
    _fields_ = [("target", _c.c_void_p), ("source", _c.c_void_p), ("sig_addr", _c.c_void_p), ("nelems", _c.c_size_t),
                ("type_size", _c.c_size_t), ("sig_op", _c.c_int), ("pe", _c.c_int)]


class SyncOp(_c.Structure):
    _fields_ = [("ivars", _c.c_void_p), ("nelems", _c.c_size_t), ("type_size", _c.c_size_t), ("status", _c.c_void_p),
                ("indices", _c.c_void_p), ("kind", _c.c_int), ("cmp", _c.c_int)]


class LockOp(_c.Structure):
    _fields_ = [("lock", _c.c_void_p)]


OPS = {"sos_rma_check": RmaOp, "sos_amo_check": AmoOp, "sos_put_signal_check": PutSignalOp,
       "sos_sync_check": SyncOp, "sos_lock_check": LockOp}


def call(lib, fn, lay, op):
    """(code, message) of check `fn` over lay = [initialized, my_pe, n_pes, mapped] and the op's fields in
    the struct's order."""
    regions = (Region * len(REGIONS))(*[Region(*r) for r in REGIONS])
    layout = Layout(lay[0], lay[1], lay[2], lay[3], len(REGIONS), regions)
    o = OPS[fn](*op)
    f = getattr(lib, fn)
    f.restype, f.argtypes = _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]
    msg = _c.create_string_buffer(MSG_LEN)
    rc = f(_c.addressof(layout), _c.addressof(o), msg, MSG_LEN)
    return rc, msg.value.decode()


def fields(cls, base, **kw):
    d = dict(base, **kw)
    return [d[name] for name, _ in cls._fields_]


def spots():
    """every region kind at its first word, its last word and one past the end, and a local address"""
    for base, size, _ in REGIONS:
        yield base, size, 0
        yield base, size, size
        yield base, size, size + 1   # marks "the last word": resolved with the word's width
    yield LOCAL, 0, 0


def at(base, size, off, width):
    return base + (size - width if off == size + 1 else off)


def reach(cls, base, name, **kw):
    """who may reach what: the PE itself and a peer, each region's first word, mapped or not"""
    for pe in (ME, OTHER):
        for mapped in (0, 1):
            for b, _, _ in REGIONS:
                yield [1, ME, N_PES, mapped], fields(cls, base, pe=pe, **{name: b}, **kw)


OK_LAYOUT = [1, ME, N_PES, 1]


def rma_cases():
    ok = OK_LAYOUT
    base = dict(remote=DEV + 64, local=LOCAL, remote_stride=8, local_stride=8, bsize=8, nblocks=1, type_size=4,
                pe=OTHER, put=1, strided=0)
    block = dict(base, bsize=4, nblocks=10)
    one = dict(base, bsize=1, remote_stride=1, local_stride=1)
    for init in (0, 1):
        for pe in (-1, ME, OTHER, N_PES):
            yield [init, ME, N_PES, 1], fields(RmaOp, base, pe=pe)
    yield [0, ME, N_PES, 1], fields(RmaOp, base, pe=9, put=0)
    yield ok, fields(RmaOp, base, pe=N_PES, put=0, remote=LOCAL)
    yield from reach(RmaOp, one, "remote")
    for put in (0, 1):
        for b, size, off in spots():
            for pe in (ME, OTHER):
                yield ok, fields(RmaOp, one, remote=at(b, size, off, 4), pe=pe, put=put)
        # the extent, not the first element, crosses the end; contiguous and in blocks
        yield ok, fields(RmaOp, base, remote=DEV + DEV_SIZE - 4 * 8 + 4, put=put)
        yield ok, fields(RmaOp, block, remote=DEV + DEV_SIZE - 4 * 76, put=put)
        yield ok, fields(RmaOp, block, remote=DEV + DEV_SIZE - 4 * 76 + 4, put=put)
        yield ok, fields(RmaOp, base, remote=DEV + 66, put=put)             # misaligned remote side
        yield ok, fields(RmaOp, base, local=LOCAL + 2, put=put)             # misaligned local side
        yield ok, fields(RmaOp, base, local=0, put=put)                     # NULL local side
        yield ok, fields(RmaOp, base, remote=LOCAL, local=0, put=put)       # ... after the symmetric check
        for strided, shape in ((0, block), (1, dict(block, bsize=1))):
            for s in (0, shape["bsize"] - 1, shape["bsize"], -1):
                yield ok, fields(RmaOp, shape, remote_stride=s, strided=strided, put=put)
                yield ok, fields(RmaOp, shape, local_stride=s, strided=strided, put=put)
            yield ok, fields(RmaOp, shape, remote_stride=0, local_stride=0, strided=strided, put=put)
        # the calling PE itself: overlap in both orders, abutting, the same bytes
        for remote, local in ((DEV, DEV + 16), (DEV + 16, DEV), (DEV, DEV + 32), (DEV + 32, DEV), (DEV, DEV)):
            yield ok, fields(RmaOp, base, remote=remote, local=local, pe=ME, put=put)
        yield ok, fields(RmaOp, block, remote=DEV, local=DEV + 16, pe=ME, put=put)
        yield ok, fields(RmaOp, block, remote=HOSTH + 16, local=HOSTH, pe=ME, put=put)
    yield ok, fields(RmaOp, base, remote=DEV, local=DEV + 16)               # a peer's are other memory
    for ts in (0, 1, 2, 3, 4, 8, 16, 32):
        yield ok, fields(RmaOp, base, type_size=ts)
    yield ok, fields(RmaOp, base, type_size=3, put=0)
    # empty ops: nothing but the PE, the element size and the strides is looked at
    for kw in (dict(bsize=0), dict(nblocks=0), dict(bsize=0, remote_stride=0, local_stride=0),
               dict(nblocks=0, remote=0, local=0), dict(nblocks=0, pe=7), dict(bsize=0, remote=LOCAL),
               dict(nblocks=0, remote_stride=2), dict(nblocks=0, local_stride=2, put=0), dict(nblocks=0, type_size=3),
               dict(bsize=0, strided=1, remote_stride=0)):
        yield ok, fields(RmaOp, block, **kw)
    # extents that do not fit a size_t
    yield ok, fields(RmaOp, block, nblocks=1 << 62)
    yield ok, fields(RmaOp, base, bsize=1 << 62, remote_stride=1 << 62, local_stride=1 << 62)
    yield ok, fields(RmaOp, block, local_stride=1 << 40, nblocks=1 << 20, remote_stride=4)
    yield ok, fields(RmaOp, block, local_stride=1 << 40, nblocks=1 << 20, remote_stride=4, put=0)


def amo_cases():
    ok = OK_LAYOUT
    base = dict(target=DEV + 64, fetch=0, type_size=8, pe=OTHER, nbi=0)
    for init in (0, 1):
        for pe in (-1, ME, OTHER, N_PES):
            yield [init, ME, N_PES, 1], fields(AmoOp, base, pe=pe)
    yield from reach(AmoOp, base, "target")
    for ts in (4, 8):
        for b, size, off in spots():
            for pe in (ME, OTHER):
                yield ok, fields(AmoOp, base, target=at(b, size, off, ts), type_size=ts, pe=pe)
        yield ok, fields(AmoOp, base, target=DEV + DEV_SIZE - ts // 2, type_size=ts)   # half past the end
        yield ok, fields(AmoOp, base, target=DEV + 64 + ts // 2, type_size=ts)          # misaligned target
        for fetch in (0, LOCAL, LOCAL + ts // 2, DEV + 128):
            yield ok, fields(AmoOp, base, fetch=fetch, nbi=1, type_size=ts)
        yield ok, fields(AmoOp, base, fetch=LOCAL + 1, nbi=0, type_size=ts)             # blocking: not looked at
        yield ok, fields(AmoOp, base, fetch=0, nbi=1, target=LOCAL, type_size=ts)       # after the symmetric check
    for ts in (0, 1, 2, 3, 16):
        yield ok, fields(AmoOp, base, type_size=ts)
        yield ok, fields(AmoOp, base, type_size=ts, target=LOCAL + 1)
        yield ok, fields(AmoOp, base, type_size=ts, target=DEV + DEV_SIZE - 1)
    yield ok, fields(AmoOp, base, target=0)


def put_signal_cases():
    ok = OK_LAYOUT
    base = dict(target=DEV + 64, source=LOCAL, sig_addr=DEV + 4096, nelems=8, type_size=8, sig_op=0, pe=OTHER)
    for init in (0, 1):
        for pe in (-1, ME, OTHER, N_PES):
            yield [init, ME, N_PES, 1], fields(PutSignalOp, base, pe=pe)
    yield from reach(PutSignalOp, base, "target")
    yield from reach(PutSignalOp, base, "sig_addr")
    for b, size, off in spots():
        for pe in (ME, OTHER):
            yield ok, fields(PutSignalOp, base, target=at(b, size, off, 8), nelems=1, pe=pe)
            yield ok, fields(PutSignalOp, base, sig_addr=at(b, size, off, 8), pe=pe)
    yield ok, fields(PutSignalOp, base, target=DEV + DEV_SIZE - 32)                    # the extent crosses the end
    yield ok, fields(PutSignalOp, base, target=HOSTH + 64, sig_addr=HOSTH + 8)        # both outside: the target is named
    yield ok, fields(PutSignalOp, base, target=HOSTH + 64, sig_addr=DATA_BASE + 8)
    for ts in (0, 1, 2, 3, 4, 8, 16, 32):
        yield ok, fields(PutSignalOp, base, type_size=ts)
    yield ok, fields(PutSignalOp, base, target=DEV + 68)                               # misaligned target
    yield ok, fields(PutSignalOp, base, source=LOCAL + 4)                              # misaligned source
    yield ok, fields(PutSignalOp, base, sig_addr=DEV + 4100)                           # misaligned signal word
    yield ok, fields(PutSignalOp, base, source=0)                                      # NULL source
    yield ok, fields(PutSignalOp, base, source=0, sig_op=7)
    yield ok, fields(PutSignalOp, base, source=0, target=LOCAL)
    for sig_op in (0, 1, 2, -1):
        yield ok, fields(PutSignalOp, base, sig_op=sig_op)
        yield ok, fields(PutSignalOp, base, sig_op=sig_op, sig_addr=LOCAL)
    # empty: only the signal
    for kw in (dict(nelems=0), dict(nelems=0, source=0, target=0), dict(nelems=0, target=LOCAL + 1, type_size=3),
               dict(nelems=0, sig_addr=HOSTH + 8), dict(nelems=0, pe=ME, sig_addr=HOSTH + 8), dict(nelems=0, sig_op=2),
               dict(nelems=0, pe=9)):
        yield ok, fields(PutSignalOp, base, **kw)
    # the signal word inside, right behind, right before and below the payload, for the PE itself and a peer
    for sig in (DEV + 64, DEV + 64 + 56, DEV + 64 + 64, DEV + 56, DEV + 48, DEV + 60):
        yield ok, fields(PutSignalOp, base, sig_addr=sig, pe=ME)
    yield ok, fields(PutSignalOp, base, sig_addr=DEV + 64 + 56, pe=ME, sig_op=7)
    yield ok, fields(PutSignalOp, base, sig_addr=DEV + 64 + 56, pe=OTHER)
    yield ok, fields(PutSignalOp, base, nelems=1 << 62)                                # no size_t holds the extent
    yield ok, fields(PutSignalOp, base, nelems=1 << 60, type_size=16)


def sync_cases():
    ok = OK_LAYOUT
    base = dict(ivars=DEV + 64, nelems=4, type_size=8, status=LOCAL, indices=LOCAL + 64, kind=SOME, cmp=4)
    # status and indices over the ivars and over each other, in both orders
    overlaps = ((DEV + 80, LOCAL + 64), (DEV + 56, LOCAL + 64), (DEV + 96, LOCAL + 64), (DEV + 48, LOCAL + 64),
                (LOCAL, DEV + 88), (LOCAL, DEV + 40), (LOCAL, DEV + 96), (LOCAL, DEV + 32), (LOCAL, LOCAL + 8),
                (LOCAL + 24, LOCAL), (LOCAL, LOCAL + 16), (LOCAL + 32, LOCAL), (LOCAL, LOCAL), (DEV + 64, DEV + 64))
    for kind in (ONE, ALL, ANY, SOME):
        n = 1 if kind == ONE else 4
        for init in (0, 1):
            for status in (0, LOCAL):
                for indices in (0, LOCAL + 64):
                    yield [init, ME, N_PES, 1], fields(SyncOp, base, kind=kind, nelems=n, status=status, indices=indices)
        yield [1, ME, N_PES, 0], fields(SyncOp, base, kind=kind, nelems=n)              # a wait needs no mapping
        yield ok, fields(SyncOp, base, kind=kind, nelems=n, ivars=DEV + DEV_SIZE - 8 * n)   # the last nelems words
        yield ok, fields(SyncOp, base, kind=kind, nelems=n, ivars=DEV + DEV_SIZE - 8 * n + 8)
        for cmp in (0, 1, 6, 7):
            yield ok, fields(SyncOp, base, kind=kind, nelems=n, cmp=cmp)
        yield ok, fields(SyncOp, base, kind=kind, nelems=n, cmp=7, ivars=DEV + 68)      # before alignment
        for status, indices in overlaps[:2] + overlaps[4:6] + overlaps[8:10] if kind in (ONE, ANY) else overlaps:
            yield ok, fields(SyncOp, base, kind=kind, nelems=n, status=status, indices=indices)
    for kind in (ONE, SOME):
        n = 1 if kind == ONE else 4
        for b, size, off in spots():
            yield ok, fields(SyncOp, base, kind=kind, nelems=1, ivars=at(b, size, off, 8))
        for ts in (0, 1, 2, 3, 4, 8, 16):
            yield ok, fields(SyncOp, base, kind=kind, nelems=n, type_size=ts)
        for ts in (2, 4, 8):
            yield ok, fields(SyncOp, base, kind=kind, nelems=n, type_size=ts, ivars=DEV + 64 + ts // 2)
    for kind in (ALL, SOME):
        for kw in (dict(), dict(indices=0, status=0), dict(ivars=LOCAL), dict(ivars=DEV + DEV_SIZE - 4), dict(cmp=9),
                   dict(ivars=DEV + DEV_SIZE)):
            yield ok, fields(SyncOp, base, kind=kind, nelems=0, **kw)
        yield ok, fields(SyncOp, base, kind=kind, nelems=1 << 62)
    yield ok, fields(SyncOp, base, ivars=0)


def lock_cases():
    yield [0, 0, 1, 1], [LOCAL + 4]
    yield [0, ME, N_PES, 0], [DEV + 64]
    for n_pes, me, mapped in ((1, 0, 0), (1, 0, 1), (N_PES, 0, 1), (N_PES, 0, 0), (N_PES, N_PES - 1, 1),
                              (N_PES, ME, 0)):
        lay = [1, me, n_pes, mapped]
        for b, size, off in spots():
            yield lay, [at(b, size, off, 8)]
        yield lay, [DEV + DEV_SIZE - 4]      # half past the end
        yield lay, [DEV + 68]                # misaligned
        yield lay, [HOSTH + 68]
        yield lay, [0]
    yield [1, 0, 2, 1], [HOSTH + 64]


GRID = [("sos_rma_check", rma_cases), ("sos_amo_check", amo_cases), ("sos_put_signal_check", put_signal_cases),
        ("sos_sync_check", sync_cases), ("sos_lock_check", lock_cases)]


def main():
    from sos_amd import shmem as S
    git = ["git", "-C", ROOT]
    dirty = subprocess.run(git + ["status", "--porcelain", "--", "sos_amd/csrc"], capture_output=True, text=True,
                           check=True).stdout.strip()
    if dirty:
        sys.exit("sos_amd/csrc differs from HEAD: the record is made from a commit's build\n" + dirty)
    commit = subprocess.run(git + ["rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    lib = S.lib()
    lines, seen = [], set()
    for fn, cases in GRID:
        for lay, op in cases():
            key = json.dumps([fn, lay, op])
            if key in seen:
                continue
            seen.add(key)
            rc, msg = call(lib, fn, lay, op)
            lines.append(json.dumps([fn, lay, op, rc, msg]))
    head = {"what": "answers of the one-sided argument checks (see make_refusals.py)", "commit": commit,
            "case": "[function, [initialized, my_pe, n_pes, mapped], the op struct's fields in order, code, message]",
            "regions": REGIONS, "msg_len": MSG_LEN}
    with open(os.path.join(HERE, "onesided_refusals.json"), "w") as f:
        f.write(json.dumps(head)[:-1] + ', "cases": [\n' + ",\n".join(lines) + "\n]}\n")
    print(f"{len(lines)} cases from {commit[:7]}")


if __name__ == "__main__":
    main()
