"""CPU: the argument check of the distributed locks (sos_lock_check, onesided_checks.cpp) as a plain
function over a made-up layout: every refusal returns its code and a message naming the
argument, in SOS's order (src/lock_c.c:44-65: initialized, `lock` symmetric over
sizeof(long)) followed by this library's own (alignment; beyond one PE the device heap, then
its mapping), the same on every PE; the texts a lock call ends the job with (a wait that ran
out, a lock word that is no lock) from their plain functions; and the kernel's C ABI refusing
bad arguments before any device work.  Nothing is started that could abort."""
import ctypes

from sos_amd import shmem as S

OK, NOT_INIT, BAD_PE, NOT_POSITIVE, NOT_SYMMETRIC, NULL_LOCAL, STRIDE, OVERLAP, PEER_HOST, NO_PATH, BAD_SIZE = range(11)
HOST_HEAP, DEVICE_HEAP, DATA, DEVICE_ALLOC = range(4)
ERR_ARG = -3
ENQUEUE, TRY, RELEASE, HANDOFF = range(4)
AWAIT_SIGNAL, AWAIT_NEXT = 0, 1


class Region(ctypes.Structure):
    _fields_ = [("base", ctypes.c_size_t), ("size", ctypes.c_size_t), ("kind", ctypes.c_int)]


class Layout(ctypes.Structure):
    _fields_ = [("initialized", ctypes.c_int), ("my_pe", ctypes.c_int), ("n_pes", ctypes.c_int),
                ("mapped", ctypes.c_int), ("nregions", ctypes.c_int), ("regions", ctypes.POINTER(Region))]


class LockOp(ctypes.Structure):
    _fields_ = [("lock", ctypes.c_void_p)]


DEV, DEV_SIZE = 0x7F0000000000, 1 << 20
HOSTH, HOSTH_SIZE = 0x500000000000, 1 << 16
DATA_BASE, DATA_SIZE = 0x600000, 4096
LOCAL = 0x10000


def check(lock=DEV + 64, initialized=1, my_pe=1, n_pes=4, mapped=1):
    regions = (Region * 3)(Region(DEV, DEV_SIZE, DEVICE_HEAP), Region(HOSTH, HOSTH_SIZE, HOST_HEAP),
                           Region(DATA_BASE, DATA_SIZE, DATA))
    lay = Layout(initialized, my_pe, n_pes, mapped, 3, regions)
    op = LockOp(lock)
    msg = ctypes.create_string_buffer(512)
    rc = S.sos_lock_check(ctypes.addressof(lay), ctypes.addressof(op), msg, 512)
    return rc, msg.value.decode()


def test_accepted_for_each_kind_of_region_on_one_pe():
    for base in (DEV, HOSTH, DATA_BASE):
        assert check(lock=base + 64, my_pe=0, n_pes=1, mapped=0) == (OK, ""), hex(base)
    assert check(lock=DEV + DEV_SIZE - 8, my_pe=0, n_pes=1) == (OK, "")     # the heap's last word
    for me in range(4):                                                      # several PEs: the device heap, mapped
        assert check(my_pe=me) == (OK, "")
    assert check(lock=DEV + DEV_SIZE - 8) == (OK, "")


def test_refusals_in_order():
    rc, msg = check(lock=LOCAL + 4, initialized=0)                           # three defects: initialized first
    assert rc == NOT_INIT and msg == "library not initialized"
    rc, msg = check(lock=LOCAL + 4)                                          # symmetric before alignment
    assert rc == NOT_SYMMETRIC and msg == f'Argument "lock" is not symmetric ({LOCAL + 4:#x})'
    rc, msg = check(lock=None)
    assert rc == NOT_SYMMETRIC and 'Argument "lock" is not symmetric' in msg
    rc, msg = check(lock=DEV + DEV_SIZE - 4)                                 # over sizeof(long), before alignment
    assert rc == NOT_SYMMETRIC and msg.startswith('Argument "lock" [') and "exceeds device sym. heap region" in msg
    rc, msg = check(lock=HOSTH + HOSTH_SIZE - 4, n_pes=1, my_pe=0)
    assert rc == NOT_SYMMETRIC and "exceeds sym. heap region" in msg
    rc, msg = check(lock=HOSTH + 68)                                         # alignment before the device-heap rule
    assert rc == BAD_SIZE and msg == f'Argument "lock" ({HOSTH + 68:#x}) must be aligned to 8 bytes'
    assert check(lock=DEV + 68, n_pes=1, my_pe=0)[0] == BAD_SIZE
    rc, msg = check(lock=HOSTH + 64, mapped=0)                               # the region before the missing mapping
    assert rc == PEER_HOST
    rc, msg = check(mapped=0)
    assert rc == NO_PATH and msg.startswith("No path to peer")


def test_device_heap_only_beyond_one_pe_on_every_pe_alike():
    for me in range(4):   # PE 0, the home of `last`, refuses what the others refuse
        for base, name in ((HOSTH, "sym. heap region"), (DATA_BASE, "sym. data region")):
            rc, msg = check(lock=base + 64, my_pe=me)
            assert rc == PEER_HOST, (me, hex(base))
            assert msg == (f'Argument "lock" ({base + 64:#x}) is in this PE\'s {name}: a lock shared by 4 PEs needs the '
                           "device symmetric heap (shmemx_malloc_device), the only memory mapped across PEs")
        assert check(my_pe=me, mapped=0)[0] == NO_PATH
    assert check(lock=HOSTH + 64, my_pe=0, n_pes=2)[0] == PEER_HOST
    assert check(lock=HOSTH + 64, my_pe=0, n_pes=1)[0] == OK


def test_expiry_message():
    msg = ctypes.create_string_buffer(512)
    S.sos_lock_expiry_message(b"shmem_set_lock", DEV + 64, AWAIT_SIGNAL, 0x00000003, 30.0, msg, 512)
    text = msg.value.decode()
    assert text.startswith(f"shmem_set_lock: lock {DEV + 64:#x} not granted after 30 s (SHMEMX_P2P_TIMEOUT)")
    assert "awaited SIGNAL (bit 31) from the predecessor" in text
    assert text.endswith("last value seen 0x00000003 (next = 3, signal = 0)")
    S.sos_lock_expiry_message(b"shmem_clear_lock", DEV + 64, AWAIT_NEXT, 0x80000000, 300.4, msg, 512)
    text = msg.value.decode()
    assert text.startswith(f"shmem_clear_lock: lock {DEV + 64:#x} not handed over after 300 s")
    assert "awaited NEXT (bits 0-30) from the successor" in text
    assert text.endswith("last value seen 0x80000000 (next = 0, signal = 1)")
    small = ctypes.create_string_buffer(16)   # truncated, terminated
    S.sos_lock_expiry_message(b"shmem_set_lock", DEV, AWAIT_SIGNAL, 0, 1.0, small, 16)
    assert small.value == b"shmem_set_lock:"
    S.sos_lock_expiry_message(b"shmem_set_lock", DEV, AWAIT_SIGNAL, 0, 1.0, None, 0)   # nowhere to write: no-op


def test_corrupt_word_message():
    msg = ctypes.create_string_buffer(256)
    S.sos_lock_corrupt_message(DEV + 64, -7, 4, msg, 256)
    assert msg.value.decode() == (f"lock word at {DEV + 64:#x} is not a lock (last/next = -7, n_pes = 4): "
                                  "was it zero-initialised?")
    S.sos_lock_corrupt_message(DEV + 64, 2**31 - 1, 2, msg, 256)
    assert "(last/next = 2147483647, n_pes = 2)" in msg.value.decode()


def test_kernel_abi_rejects_bad_args_without_gpu():
    f = S.sosx_lock_step
    a = 1 << 20   # never dereferenced: every argument is checked before any device work
    last, mine, table, res = a, a + 68, a + 128, a + 256

    def step(kind=ENQUEUE, last=last, mine=mine, table=table, offset=4, me=1, n_pes=4, res=res):
        return f(kind, last, mine, table, offset, me, n_pes, res, None)

    for kind in (-1, 4, 99):
        assert step(kind=kind) == ERR_ARG, kind
    for k in ("last", "mine", "table", "res"):
        assert step(**{k: None}) == ERR_ARG, k                               # null
    assert step(last=a + 2) == ERR_ARG and step(mine=a + 70) == ERR_ARG      # misaligned words
    assert step(table=a + 132) == ERR_ARG and step(res=a + 260) == ERR_ARG   # misaligned table and record
    assert step(offset=6) == ERR_ARG
    for me, n in ((-1, 4), (4, 4), (0, 0), (1, 1), (0, -3)):
        assert step(me=me, n_pes=n) == ERR_ARG, (me, n)
    for kind in (TRY, RELEASE, HANDOFF):
        assert step(kind=kind, me=7, n_pes=4) == ERR_ARG
    n = ctypes.c_int(-1)
    assert S.sosx_lock_table(ctypes.byref(n)) is None and n.value == 0       # nothing was set up or launched
    steps, probes = ctypes.c_long(-1), ctypes.c_long(-1)
    S.sosx_lock_stats(ctypes.byref(steps), ctypes.byref(probes))
    assert (steps.value, probes.value) == (0, 0)
