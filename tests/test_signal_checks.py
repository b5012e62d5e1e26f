"""CPU: the argument checks of put-with-signal and of the waits and tests
(sos_put_signal_check, sos_sync_check, onesided_checks.cpp) as plain functions over a made-up
layout: every refusal returns its code and a message naming the argument, in SOS's order
(src/data_c.c4:691-699: initialized, PE, target symmetric, source NULL, overlap for
pe == my_pe, sig_op; src/synchronization_c.c4: initialized, ivars symmetric, the overlaps,
the comparison) followed by this library's own, and the kernels' C ABI refuses bad
arguments before any device work.  Nothing is started that could abort."""
import ctypes

import pytest

from sos_amd import shmem as S

OK, NOT_INIT, BAD_PE, NOT_POSITIVE, NOT_SYMMETRIC, NULL_LOCAL, STRIDE, OVERLAP, PEER_HOST, NO_PATH, BAD_SIZE, \
    NULL_FETCH, BAD_SIG_OP, BAD_CMP = range(14)
HOST_HEAP, DEVICE_HEAP, DATA, DEVICE_ALLOC = range(4)
ONE, ALL, ANY, SOME = range(4)
ERR_ARG = -3


class Region(ctypes.Structure):
    _fields_ = [("base", ctypes.c_size_t), ("size", ctypes.c_size_t), ("kind", ctypes.c_int)]


class Layout(ctypes.Structure):
    _fields_ = [("initialized", ctypes.c_int), ("my_pe", ctypes.c_int), ("n_pes", ctypes.c_int),
                ("mapped", ctypes.c_int), ("nregions", ctypes.c_int), ("regions", ctypes.POINTER(Region))]


class PutOp(ctypes.Structure):
    _fields_ = [("target", ctypes.c_void_p), ("source", ctypes.c_void_p), ("sig_addr", ctypes.c_void_p),
                ("nelems", ctypes.c_size_t), ("type_size", ctypes.c_size_t), ("sig_op", ctypes.c_int), ("pe", ctypes.c_int)]


class SyncOp(ctypes.Structure):
    _fields_ = [("ivars", ctypes.c_void_p), ("nelems", ctypes.c_size_t), ("type_size", ctypes.c_size_t),
                ("status", ctypes.c_void_p), ("indices", ctypes.c_void_p), ("kind", ctypes.c_int), ("cmp", ctypes.c_int)]


class RmaOp(ctypes.Structure):  # sos_rma_op, for the put that shares a reason text
    _fields_ = [("remote", ctypes.c_void_p), ("local", ctypes.c_void_p),
                ("remote_stride", ctypes.c_ssize_t), ("local_stride", ctypes.c_ssize_t),
                ("bsize", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("type_size", ctypes.c_size_t),
                ("pe", ctypes.c_int), ("put", ctypes.c_int), ("strided", ctypes.c_int)]


DEV, DEV_SIZE = 0x7F0000000000, 1 << 20
HOSTH, HOSTH_SIZE = 0x500000000000, 1 << 16
DATA_BASE, DATA_SIZE = 0x600000, 4096
LOCAL = 0x10000


def check(fn, op, initialized=1, my_pe=1, n_pes=4, mapped=1):
    regions = (Region * 3)(Region(DEV, DEV_SIZE, DEVICE_HEAP), Region(HOSTH, HOSTH_SIZE, HOST_HEAP),
                           Region(DATA_BASE, DATA_SIZE, DATA))
    lay = Layout(initialized, my_pe, n_pes, mapped, 3, regions)
    msg = ctypes.create_string_buffer(512)
    rc = fn(ctypes.addressof(lay), ctypes.addressof(op), msg, 512)
    return rc, msg.value.decode()


def put(target=DEV + 64, source=LOCAL, sig=DEV + 4096, nelems=8, ts=8, sig_op=0, pe=2, **kw):
    return check(S.sos_put_signal_check, PutOp(target, source, sig, nelems, ts, sig_op, pe), **kw)


def sync(ivars=DEV + 64, nelems=4, ts=8, status=LOCAL, indices=LOCAL + 64, kind=SOME, cmp=4, **kw):
    return check(S.sos_sync_check, SyncOp(ivars, nelems, ts, status, indices, kind, cmp), **kw)


def test_put_signal_accepted_for_each_kind_of_region():
    assert put() == (OK, "")
    assert put(sig_op=1, ts=16, nelems=3, target=DEV + 16, source=LOCAL + 16) == (OK, "")
    assert put(nelems=0, source=None) == (OK, "")                      # only the signal
    assert put(target=DEV + DEV_SIZE - 64, nelems=8) == (OK, "")       # the heap's last bytes
    for base in (DEV, HOSTH, DATA_BASE):                                 # the PE itself: any symmetric memory
        assert put(target=base + 64, sig=base + 1024, pe=1, mapped=0) == (OK, ""), hex(base)


def test_put_signal_refusals_in_order():
    rc, msg = put(pe=9, target=LOCAL, initialized=0)
    assert rc == NOT_INIT and "not initialized" in msg
    rc, msg = put(pe=4, target=LOCAL)                                   # two defects: the PE is reported
    assert rc == BAD_PE and msg == "PE argument (4) is invalid"
    rc, msg = put(target=LOCAL, source=None)                            # symmetric before NULL
    assert rc == NOT_SYMMETRIC and msg == f'Argument "target" is not symmetric ({LOCAL:#x})'
    rc, msg = put(target=DEV + DEV_SIZE - 32)
    assert rc == NOT_SYMMETRIC and 'Argument "target"' in msg and "exceeds device sym. heap region" in msg
    rc, msg = put(source=None, sig_op=7)                                # NULL before sig_op
    assert rc == NULL_LOCAL and msg == 'Argument "source" is NULL'
    rc, msg = put(pe=1, sig=DEV + 64 + 56, sig_op=7)                    # overlap before sig_op
    assert rc == OVERLAP and msg.startswith('Argument "target" [') and "overlaps argument" in msg
    assert put(pe=1, sig=DEV + 64 + 64)[0] == OK                        # right behind the payload
    assert put(pe=2, sig=DEV + 64 + 56)[0] == OK                        # SOS checks it for pe == my_pe only
    rc, msg = put(sig_op=2, sig=LOCAL)                                  # sig_op before this library's own
    assert rc == BAD_SIG_OP and msg == 'Argument "sig_op", invalid atomic operation for signal (2)'
    assert put(sig_op=-1)[0] == BAD_SIG_OP


def test_put_signal_own_checks():
    rc, msg = put(sig=LOCAL)
    assert rc == NOT_SYMMETRIC and msg == f'Argument "sig_addr" is not symmetric ({LOCAL:#x})'
    rc, msg = put(sig=DEV + DEV_SIZE - 4)
    assert rc == NOT_SYMMETRIC and 'Argument "sig_addr"' in msg and "exceeds" in msg
    rc, msg = put(sig=DEV + 4100)
    assert rc == BAD_SIZE and msg == f'Argument "sig_addr" ({DEV + 4100:#x}) must be aligned to 8 bytes'
    assert put(ts=3)[0] == BAD_SIZE and put(target=DEV + 68)[0] == BAD_SIZE
    rc, msg = put(sig=HOSTH + 8)
    assert rc == PEER_HOST and 'Argument "sig_addr"' in msg and "needs the device symmetric heap" in msg
    rc, msg = put(target=HOSTH + 64, sig=HOSTH + 8)
    assert rc == PEER_HOST and 'Argument "target"' in msg
    # the reason text is put / get's
    rop = RmaOp(HOSTH + 64, LOCAL, 1, 1, 1, 1, 8, 2, 1, 0)
    f = S.lib().sos_rma_check
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    assert check(f, rop) == (PEER_HOST, msg)
    assert put(target=HOSTH + 64, mapped=0)[0] == PEER_HOST            # before the missing mapping
    rc, msg = put(mapped=0)
    assert rc == NO_PATH and msg.startswith("No path to peer")


def test_sync_accepted():
    assert sync() == (OK, "")
    assert sync(status=None) == (OK, "") and sync(kind=ALL, indices=None) == (OK, "")
    assert sync(kind=ONE, nelems=1, status=None, indices=None, ts=2, ivars=HOSTH + 2) == (OK, "")
    assert sync(kind=ANY, ts=4, ivars=DATA_BASE + 4, indices=None) == (OK, "")
    assert sync(nelems=0, indices=None) == (OK, "")
    assert sync(ivars=DEV + DEV_SIZE - 32) == (OK, "")


def test_sync_refusals_in_order():
    rc, msg = sync(ivars=LOCAL, initialized=0)
    assert rc == NOT_INIT and "not initialized" in msg
    rc, msg = sync(ivars=LOCAL + 4096, cmp=9)                           # two defects: symmetric is reported
    assert rc == NOT_SYMMETRIC and msg == f'Argument "ivars" is not symmetric ({LOCAL + 4096:#x})'
    rc, msg = sync(ivars=LOCAL + 4096, kind=ONE, nelems=1)
    assert rc == NOT_SYMMETRIC and msg.startswith('Argument "ivar" ')
    rc, msg = sync(ivars=DEV + DEV_SIZE - 16)                           # the probes read all nelems
    assert rc == NOT_SYMMETRIC and "exceeds device sym. heap region" in msg
    rc, msg = sync(indices=LOCAL + 8, cmp=9)                            # the overlaps before the comparison
    assert rc == OVERLAP and msg.startswith('Argument "indices" [')
    rc, msg = sync(status=DEV + 80)
    assert rc == OVERLAP and msg.startswith('Argument "ivars" [')
    assert sync(indices=DEV + 56)[0] == OVERLAP
    assert sync(indices=DEV + 56, kind=ANY)[0] == OK                    # only _some has indices
    for cmp in (0, 7, -1):
        rc, msg = sync(cmp=cmp, ivars=DEV + 68)                         # before this library's alignment check
        assert rc == BAD_CMP and msg == f'Argument "cmp", invalid comparison operation ({cmp})'
    rc, msg = sync(ivars=DEV + 68)
    assert rc == BAD_SIZE and msg == f'Argument "ivars" ({DEV + 68:#x}) must be aligned to the element size 8'
    assert sync(ivars=DEV + 68, ts=4)[0] == OK and sync(ivars=DEV + 66, ts=2)[0] == OK
    assert sync(ts=1)[0] == BAD_SIZE and sync(ts=16)[0] == BAD_SIZE
    assert sync(indices=None)[0] == NULL_LOCAL


def test_kernel_abi_rejects_bad_args_without_gpu():
    f, g = S.sosx_put_signal, S.sosx_sync_snapshot
    a = 1 << 20  # never dereferenced: every argument is checked before any device work
    assert f(a, a + 64, 8, None, 1, 0, None) == ERR_ARG          # null sig_addr
    assert f(a, a + 64, 8, a + 132, 1, 0, None) == ERR_ARG       # misaligned sig_addr
    assert f(a, a + 64, 8, a + 128, 1, 2, None) == ERR_ARG       # unknown sig_op
    assert f(None, a + 64, 8, a + 128, 1, 0, None) == ERR_ARG and f(a, None, 8, a + 128, 1, 1, None) == ERR_ARG
    assert g(a, a + 64, 4, 3, None) == ERR_ARG and g(None, a, 4, 4, None) == ERR_ARG and g(a, None, 4, 8, None) == ERR_ARG
    assert g(a, a + 2, 4, 4, None) == ERR_ARG and g(a, a, 0, 8, None) == 0
    assert S.sosx_put_signal_ticket() is None                    # nothing was launched


@pytest.mark.parametrize("n,dmis,smis,want", [
    (0, 0, 0, (16, 0, 0, 0, 0, 0, 1)), (4096, 0, 0, (16, 0, 0, 256, 0, 1, 1)), (100, 5, 5, (16, 0, 11, 5, 9, 1, 1)),
    (100, 4, 12, (16, 1, 12, 5, 8, 1, 1)), (100, 3, 8, (1, 0, 0, 100, 0, 1, 1)), (100, 2, 8, (2, 0, 0, 50, 0, 1, 1)),
    (9, 9, 9, (16, 0, 7, 0, 2, 0, 1)), (3, 14, 14, (16, 0, 2, 0, 1, 0, 1))])
def test_put_signal_plan(n, dmis, smis, want):
    out = (ctypes.c_longlong * 8)()
    assert S.sosx_put_signal_plan((1 << 30) + dmis, (1 << 31) + smis, n, out) == 0
    assert tuple(out)[:7] == want and out[7] == 256
