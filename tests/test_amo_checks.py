"""CPU: the argument checks of the atomic entries (sos_amo_check, onesided_checks.cpp) as a plain
function over a made-up layout: each refusal returns its code and its message, in SOS's
order (src/atomic_c.c4: initialized, PE, symmetric over sizeof(TYPE)), and the kernel's C
ABI (sosx_amo) refuses bad arguments before any device work.  Nothing is started that
could abort."""
import ctypes

import pytest

from sos_amd import shmem as S

OK, NOT_INIT, BAD_PE, NOT_POSITIVE, NOT_SYMMETRIC, NULL_LOCAL, STRIDE, OVERLAP, PEER_HOST, NO_PATH, BAD_SIZE, \
    NULL_FETCH = range(12)
HOST_HEAP, DEVICE_HEAP, DATA, DEVICE_ALLOC = range(4)
SET, FETCH, SWAP, CSWAP, ADD, AND, OR, XOR = range(8)
ERR_OP, ERR_ARG = -2, -3


class Region(ctypes.Structure):
    _fields_ = [("base", ctypes.c_size_t), ("size", ctypes.c_size_t), ("kind", ctypes.c_int)]


class Layout(ctypes.Structure):
    _fields_ = [("initialized", ctypes.c_int), ("my_pe", ctypes.c_int), ("n_pes", ctypes.c_int),
                ("mapped", ctypes.c_int), ("nregions", ctypes.c_int), ("regions", ctypes.POINTER(Region))]


class Op(ctypes.Structure):
    _fields_ = [("target", ctypes.c_void_p), ("fetch", ctypes.c_void_p), ("type_size", ctypes.c_size_t),
                ("pe", ctypes.c_int), ("nbi", ctypes.c_int)]


class RmaOp(ctypes.Structure):  # sos_rma_op, for the put that shares a reason text
    _fields_ = [("remote", ctypes.c_void_p), ("local", ctypes.c_void_p),
                ("remote_stride", ctypes.c_ssize_t), ("local_stride", ctypes.c_ssize_t),
                ("bsize", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("type_size", ctypes.c_size_t),
                ("pe", ctypes.c_int), ("put", ctypes.c_int), ("strided", ctypes.c_int)]


DEV, DEV_SIZE = 0x7F0000000000, 1 << 20       # the device heap of the made-up layout
HOSTH, HOSTH_SIZE = 0x500000000000, 1 << 16   # its host heap
DATA_BASE, DATA_SIZE = 0x600000, 4096
LOCAL = 0x10000                               # a private (non-symmetric) address


def check(op, initialized=1, my_pe=1, n_pes=4, mapped=1):
    regions = (Region * 3)(Region(DEV, DEV_SIZE, DEVICE_HEAP), Region(HOSTH, HOSTH_SIZE, HOST_HEAP),
                           Region(DATA_BASE, DATA_SIZE, DATA))
    lay = Layout(initialized, my_pe, n_pes, mapped, 3, regions)
    msg = ctypes.create_string_buffer(512)
    rc = S.lib().sos_amo_check(ctypes.addressof(lay), ctypes.addressof(op), msg, 512)
    return rc, msg.value.decode()


def amo(target=DEV + 64, fetch=None, ts=8, pe=2, nbi=0):
    return Op(target, fetch, ts, pe, nbi)


def test_accepts_plain_operations():
    assert check(amo()) == (OK, "")
    assert check(amo(ts=4, target=DEV + 4)) == (OK, "")
    assert check(amo(fetch=LOCAL, nbi=1)) == (OK, "")
    # the last word of the heap
    assert check(amo(target=DEV + DEV_SIZE - 8)) == (OK, "")
    # the calling PE itself: any symmetric memory, no mapping needed
    assert check(amo(target=HOSTH + 8, pe=1), mapped=0) == (OK, "")
    assert check(amo(target=DATA_BASE + 16, pe=1), mapped=0) == (OK, "")
    # the blocking forms never look at `fetch`
    assert check(amo(fetch=None, nbi=0)) == (OK, "")


def test_not_initialized_comes_first():
    rc, msg = check(amo(pe=99, target=LOCAL), initialized=0)
    assert rc == NOT_INIT and "not initialized" in msg


@pytest.mark.parametrize("pe", [-1, 4, 1 << 20])
def test_pe_out_of_range(pe):
    rc, msg = check(amo(pe=pe, target=0x1234))  # before the symmetric check
    assert rc == BAD_PE and msg == f"PE argument ({pe}) is invalid"


def test_target_not_symmetric():
    rc, msg = check(amo(target=LOCAL))
    assert rc == NOT_SYMMETRIC and msg == f'Argument "target" is not symmetric ({LOCAL:#x})'
    assert check(amo(target=None))[0] == NOT_SYMMETRIC
    assert check(amo(target=DEV + DEV_SIZE))[0] == NOT_SYMMETRIC  # one past the end
    # before the size and alignment checks, as SOS has nothing after it
    assert check(amo(target=LOCAL + 1, ts=3))[0] == NOT_SYMMETRIC


def test_target_runs_over_the_regions_end():
    rc, msg = check(amo(target=DEV + DEV_SIZE - 4, ts=8))
    assert rc == NOT_SYMMETRIC and "exceeds device sym. heap region" in msg and f"{DEV + DEV_SIZE:#x})" in msg
    assert check(amo(target=DEV + DEV_SIZE - 4, ts=4))[0] == OK
    rc, msg = check(amo(target=HOSTH + HOSTH_SIZE - 4, ts=8, pe=1))
    assert rc == NOT_SYMMETRIC and "exceeds sym. heap region" in msg
    rc, msg = check(amo(target=DATA_BASE + DATA_SIZE - 2, ts=4, pe=1))
    assert rc == NOT_SYMMETRIC and "exceeds sym. data region" in msg


def test_target_alignment():
    rc, msg = check(amo(target=DEV + 4, ts=8))
    assert rc == BAD_SIZE and msg == f'Argument "target" ({DEV + 4:#x}) must be aligned to the element size 8'
    assert check(amo(target=DEV + 2, ts=4))[0] == BAD_SIZE
    assert check(amo(target=DEV + 4, ts=4))[0] == OK


@pytest.mark.parametrize("ts", [0, 1, 2, 3, 16])
def test_type_size_is_4_or_8(ts):
    rc, msg = check(amo(target=DEV + 64, ts=ts))
    assert rc == BAD_SIZE and msg == f"element size {ts} is not 4 or 8"


def test_nbi_needs_a_fetch():
    rc, msg = check(amo(nbi=1, fetch=None))
    assert rc == NULL_FETCH and msg == 'Argument "fetch" is NULL'
    assert check(amo(nbi=1, fetch=LOCAL + 4, ts=8))[0] == BAD_SIZE
    assert check(amo(nbi=1, fetch=LOCAL + 4, ts=4))[0] == OK
    # after the symmetric check
    assert check(amo(nbi=1, fetch=None, target=LOCAL))[0] == NOT_SYMMETRIC


def test_peer_target_outside_the_device_heap():
    rc, msg = check(amo(target=HOSTH + 64, pe=2))
    assert rc == PEER_HOST and f"{HOSTH + 64:#x}" in msg and "needs the device symmetric heap" in msg
    # the reason text is put / get's
    rop = RmaOp(HOSTH + 64, LOCAL, 1, 1, 1, 1, 8, 2, 1, 0)
    regions = (Region * 1)(Region(HOSTH, HOSTH_SIZE, HOST_HEAP))
    lay = Layout(1, 1, 4, 1, 1, regions)
    f = S.lib().sos_rma_check
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    rmsg = ctypes.create_string_buffer(512)
    assert f(ctypes.addressof(lay), ctypes.addressof(rop), rmsg, 512) == PEER_HOST
    assert rmsg.value.decode() == msg
    rc, msg = check(amo(target=DATA_BASE, pe=0))
    assert rc == PEER_HOST and "sym. data region" in msg
    # reported before the missing mapping
    assert check(amo(target=HOSTH + 64, pe=2), mapped=0)[0] == PEER_HOST


def test_no_mapping():
    rc, msg = check(amo(), mapped=0)
    assert rc == NO_PATH and msg.startswith("No path to peer")
    assert check(amo(pe=1), mapped=0)[0] == OK  # the calling PE needs none


def test_kernel_abi_rejects_bad_args_without_gpu():
    f = S.sosx_amo
    a = 1 << 20  # never dereferenced: every argument is checked before any device work
    assert f(ADD, None, 1, 0, None, 8, 0, None) == ERR_ARG          # null target
    assert f(ADD, a + 4, 1, 0, None, 8, 0, None) == ERR_ARG         # misaligned target
    assert f(ADD, a + 2, 1, 0, None, 4, 0, None) == ERR_ARG
    assert f(ADD, a, 1, 0, a + 8 + 4, 8, 0, None) == ERR_ARG        # misaligned fetch
    assert f(ADD, a, 1, 0, None, 3, 0, None) == ERR_ARG             # width 3
    assert f(ADD, a, 1, 0, None, 16, 0, None) == ERR_ARG
    assert f(8, a, 1, 0, None, 8, 0, None) == ERR_ARG               # no such op
    assert f(-1, a, 1, 0, None, 8, 0, None) == ERR_ARG
    assert f(FETCH, a, 0, 0, None, 8, 0, None) == ERR_ARG           # a load with nowhere to put it
    for op in (CSWAP, ADD, AND, OR, XOR):                           # not defined on floats
        assert f(op, a, 1, 0, None, 4, 1, None) == ERR_OP, op
        assert f(op, a, 1, 0, None, 8, 1, None) == ERR_OP, op
