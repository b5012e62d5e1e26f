"""CPU: the argument checks of the one-sided entries (sos_rma_check, onesided_checks.cpp) as a plain
function: each refusal returns its code and its message, in SOS's order
(src/data_c.c4:300-680), and nothing is started that could abort."""
import ctypes

import pytest

from sos_amd import shmem as S

OK, NOT_INIT, BAD_PE, NOT_POSITIVE, NOT_SYMMETRIC, NULL_LOCAL, STRIDE, OVERLAP, PEER_HOST, NO_PATH, BAD_SIZE = range(11)
HOST_HEAP, DEVICE_HEAP, DATA, DEVICE_ALLOC = range(4)


class Region(ctypes.Structure):
    _fields_ = [("base", ctypes.c_size_t), ("size", ctypes.c_size_t), ("kind", ctypes.c_int)]


class Layout(ctypes.Structure):
    _fields_ = [("initialized", ctypes.c_int), ("my_pe", ctypes.c_int), ("n_pes", ctypes.c_int),
                ("mapped", ctypes.c_int), ("nregions", ctypes.c_int), ("regions", ctypes.POINTER(Region))]


class Op(ctypes.Structure):
    _fields_ = [("remote", ctypes.c_void_p), ("local", ctypes.c_void_p),
                ("remote_stride", ctypes.c_ssize_t), ("local_stride", ctypes.c_ssize_t),
                ("bsize", ctypes.c_size_t), ("nblocks", ctypes.c_size_t), ("type_size", ctypes.c_size_t),
                ("pe", ctypes.c_int), ("put", ctypes.c_int), ("strided", ctypes.c_int)]


DEV, DEV_SIZE = 0x7F0000000000, 1 << 20       # the device heap of the made-up layout
HOSTH, HOSTH_SIZE = 0x500000000000, 1 << 16   # its host heap
DATA_BASE, DATA_SIZE = 0x600000, 4096
LOCAL = 0x10000                               # a private (non-symmetric) local buffer


def check(op, initialized=1, my_pe=1, n_pes=4, mapped=1):
    regions = (Region * 3)(Region(DEV, DEV_SIZE, DEVICE_HEAP), Region(HOSTH, HOSTH_SIZE, HOST_HEAP),
                           Region(DATA_BASE, DATA_SIZE, DATA))
    lay = Layout(initialized, my_pe, n_pes, mapped, 3, regions)
    f = S.lib().sos_rma_check
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(Layout), ctypes.POINTER(Op), ctypes.c_char_p, ctypes.c_size_t]
    msg = ctypes.create_string_buffer(512)
    rc = f(ctypes.byref(lay), ctypes.byref(op), msg, 512)
    return rc, msg.value.decode()


def put(remote=DEV, local=LOCAL, nelems=8, ts=4, pe=2):
    return Op(remote, local, nelems, nelems, nelems, 1, ts, pe, 1, 0)


def ibput(remote=DEV, local=LOCAL, tst=8, sst=8, bsize=4, nblocks=10, ts=4, pe=2, put_=1):
    return Op(remote, local, tst if put_ else sst, sst if put_ else tst, bsize, nblocks, ts, pe, put_, 0)


def test_accepts_a_plain_put_get_and_block_forms():
    assert check(put()) == (OK, "")
    assert check(Op(DEV, LOCAL, 8, 8, 8, 1, 4, 2, 0, 0)) == (OK, "")  # get
    assert check(ibput()) == (OK, "")
    assert check(ibput(put_=0)) == (OK, "")
    assert check(Op(DEV, LOCAL, 3, 1, 1, 100, 8, 0, 1, 1)) == (OK, "")  # iput
    # the calling PE itself: any symmetric memory, no mapping needed
    assert check(put(remote=HOSTH, pe=1), mapped=0) == (OK, "")
    assert check(put(remote=DATA_BASE + 8, pe=1), mapped=0) == (OK, "")


def test_not_initialized_comes_first():
    rc, msg = check(put(pe=99), initialized=0)
    assert rc == NOT_INIT and "not initialized" in msg


@pytest.mark.parametrize("pe", [-1, 4, 1 << 20])
def test_pe_out_of_range(pe):
    rc, msg = check(put(pe=pe, remote=0x1234))  # before the symmetric check
    assert rc == BAD_PE and msg == f"PE argument ({pe}) is invalid"


def test_remote_not_symmetric():
    rc, msg = check(put(remote=LOCAL, local=DEV))
    assert rc == NOT_SYMMETRIC and msg == f'Argument "target" is not symmetric ({LOCAL:#x})'
    rc, msg = check(Op(LOCAL, DEV, 8, 8, 8, 1, 4, 2, 0, 0))
    assert rc == NOT_SYMMETRIC and msg.startswith('Argument "source" is not symmetric')


def test_remote_extent_past_the_heap_by_one_element():
    n = 1000
    fits = put(remote=DEV + DEV_SIZE - 4 * n, nelems=n)
    assert check(fits)[0] == OK
    rc, msg = check(put(remote=DEV + DEV_SIZE - 4 * n, nelems=n + 1))
    assert rc == NOT_SYMMETRIC and "exceeds device sym. heap region" in msg and f"{DEV + DEV_SIZE:#x})" in msg
    # block form: the extent is (nblocks - 1) * stride + bsize elements
    ext = (10 - 1) * 8 + 4
    assert check(ibput(remote=DEV + DEV_SIZE - 4 * ext))[0] == OK
    rc, msg = check(ibput(remote=DEV + DEV_SIZE - 4 * ext + 4))
    assert rc == NOT_SYMMETRIC and "exceeds" in msg
    # the get's remote side is the source, with the source's stride
    assert check(ibput(remote=DEV + DEV_SIZE - 4 * ext, put_=0))[0] == OK
    assert check(ibput(remote=DEV + DEV_SIZE - 4 * ext + 4, put_=0))[0] == NOT_SYMMETRIC
    # the host heap's end, for the calling PE
    rc, msg = check(put(remote=HOSTH + HOSTH_SIZE - 4, nelems=2, pe=1))
    assert rc == NOT_SYMMETRIC and "exceeds sym. heap region" in msg


def test_null_local_side():
    rc, msg = check(put(local=None))
    assert rc == NULL_LOCAL and msg == 'Argument "source" is NULL'
    rc, msg = check(Op(DEV, None, 8, 8, 8, 1, 4, 2, 0, 0))
    assert rc == NULL_LOCAL and msg == 'Argument "target" is NULL'
    # checked after the symmetric check, as SOS does
    assert check(put(remote=LOCAL, local=None))[0] == NOT_SYMMETRIC


def test_zero_length_is_accepted_and_checks_nothing_else():
    assert check(put(remote=0x1234, local=None, nelems=0)) == (OK, "")
    assert check(ibput(remote=None, local=None, nblocks=0)) == (OK, "")
    assert check(ibput(remote=None, local=None, bsize=0, tst=0, sst=0)) == (OK, "")
    assert check(put(nelems=0, pe=7))[0] == BAD_PE  # the PE is still checked


def test_stride_less_than_block():
    rc, msg = check(ibput(tst=3))
    assert rc == STRIDE and msg == 'Stride argument "tst" (3), is less than block size 4'
    rc, msg = check(ibput(sst=2))
    assert rc == STRIDE and msg == 'Stride argument "sst" (2), is less than block size 4'
    rc, msg = check(ibput(sst=2, put_=0))  # ibget: sst is the remote side's
    assert rc == STRIDE and '"sst" (2)' in msg
    assert check(ibput(tst=-1, remote=DEV))[0] == STRIDE
    assert check(ibput(tst=4, sst=4))[0] == OK  # stride == bsize is allowed


def test_iput_strides_must_be_positive():
    rc, msg = check(Op(DEV, LOCAL, 0, 1, 1, 10, 4, 2, 1, 1))
    assert rc == NOT_POSITIVE and msg == "Argument tst must be positive (0)"
    rc, msg = check(Op(DEV, LOCAL, 1, -2, 1, 10, 4, 2, 1, 1))
    assert rc == NOT_POSITIVE and msg == "Argument sst must be positive (-2)"


def test_self_overlap():
    rc, msg = check(put(remote=DEV, local=DEV + 16, pe=1))  # 8 floats: [0, 32) and [16, 48)
    assert rc == OVERLAP and "overlaps argument" in msg
    assert check(put(remote=DEV, local=DEV + 32, pe=1))[0] == OK  # abutting
    assert check(put(remote=DEV, local=DEV, pe=1))[0] == OVERLAP  # complete overlap is not allowed
    # interleaved block extents overlap although no block does
    assert check(ibput(remote=DEV, local=DEV + 16, pe=1))[0] == OVERLAP
    # another PE's copy of the same addresses is other memory
    assert check(put(remote=DEV, local=DEV + 16, pe=2))[0] == OK


def test_peer_host_heap_address():
    rc, msg = check(put(remote=HOSTH + 64, pe=2))
    assert rc == PEER_HOST and f"{HOSTH + 64:#x}" in msg and "needs the device symmetric heap" in msg
    rc, msg = check(put(remote=DATA_BASE, pe=0))
    assert rc == PEER_HOST and "sym. data region" in msg
    # reported before the missing mapping
    assert check(put(remote=HOSTH + 64, pe=2), mapped=0)[0] == PEER_HOST


def test_no_mapping():
    rc, msg = check(put(), mapped=0)
    assert rc == NO_PATH and msg.startswith("No path to peer")
    assert check(Op(DEV, LOCAL, 8, 8, 8, 1, 4, 3, 0, 0), mapped=0)[0] == NO_PATH  # get
    assert check(put(pe=1, local=LOCAL), mapped=0)[0] == OK  # the calling PE needs none


def test_element_size_and_alignment():
    assert check(put(ts=3))[0] == BAD_SIZE
    assert check(put(remote=DEV + 2, ts=4))[0] == BAD_SIZE


def test_shmem_ptr_is_null_before_init():
    assert S.lib().shmem_ptr(DEV, 0) is None
