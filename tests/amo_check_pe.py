"""Multi-PE correctness run of the atomic memory operations (one process per PE,
tools/oshrun, p2p transport): every shmem_<T>_atomic_* form once per width class between
each PE and itself, (me + 1) % n and (me - 1) % n, then the contended cases -- a shared
fetch-add counter, an unsynchronised add burst, a compare-swap claim word -- the nbi forms
with `fetch` in device, pinned and pageable memory (more outstanding than the library's
ring holds), and self-PE targets on the host heap.

Every expected value is plain Python integer arithmetic at the type's width (floats only as
bit patterns).  Phases are separated by shmem_barrier_all only; nothing waits on memory.
At the end the library's count of peer reads that followed a wait without an acquire
(sosx_acquire_stats) must be 0.

Prints one line per PE, exit 0 = OK.
"""
import ctypes
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sos_amd import _lib as L  # noqa: E402
from sos_amd import shmem as S  # noqa: E402
from tests import readback as R  # noqa: E402

# type -> (bits, signed)
INTS = {"int": (32, True), "long": (64, True), "uint64": (64, False), "size": (64, False), "uint32": (32, False)}
FLOATS = {"float": 32, "double": 64}
K_CONTENDED = 64      # blocking fetch-adds per PE on the shared counter
K_BURST = 256         # non-fetching adds per PE with no sync in between
N_NBI = 100           # outstanding nbi calls before one quiet: more than the ring's 64 slots
NAN32, NAN64 = 0x7FC12345, 0x7FF80000DEADBEEF   # quiet NaNs with payloads
NEG0_32, NEG0_64 = 0x80000000, 0x8000000000000000


def wrap(v, bits, signed):
    """v at the type's width, as the Python int ctypes passes and returns."""
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def f_from_bits(b, bits):
    return struct.unpack("<f" if bits == 32 else "<d", struct.pack("<I" if bits == 32 else "<Q", b))[0]


def f_bits(x, bits):
    return struct.unpack("<I" if bits == 32 else "<Q", struct.pack("<f" if bits == 32 else "<d", x))[0]


def acquire_stats():
    a, r, u = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    L.lib().sosx_acquire_stats(ctypes.byref(a), ctypes.byref(r), ctypes.byref(u), None)
    return a.value, r.value, u.value


def main():
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    torch.cuda.set_device(S.lib().shmemx_get_device())
    world = S.team_world()
    right, left = (me + 1) % P, (me - 1) % P
    bad, checks = [], 0
    words = S.shmemx_malloc_device(8 * 256)    # 8-byte slots peers operate on
    gathered = S.shmemx_malloc_device(8 * K_CONTENDED * P)
    mine = S.shmemx_malloc_device(8 * K_CONTENDED)
    S.shmem_barrier_all()

    def expect(want, got, what):
        nonlocal checks
        checks += 1
        if want != got:
            bad.append((what, "want", want, "got", got))

    # slot of case c as seen from the PE that operates on it: 0 itself, 1 the right
    # neighbour's word (written by its left), 2 the left neighbour's word
    def slot(c, k):
        return words + 8 * (3 * c + k)

    targets = ((0, me), (1, right), (2, left))

    def init_of(owner, c, k, bits):
        return (0x1111 * (owner + 1) + 0x101 * c + k + (0x7A000000 << (bits - 32))) & ((1 << bits) - 1)

    # ---- every integer op once per width class ---------------------------------------------------
    for ty, (bits, signed) in INTS.items():
        fn = lambda form: getattr(S, f"shmem_{ty}_{form}")  # noqa: E731
        put, get = getattr(S, f"shmem_{ty}_p"), getattr(S, f"shmem_{ty}_g")
        w = lambda v: wrap(v, bits, signed)  # noqa: E731
        top = (1 << (bits - 1)) - 1 if signed else (1 << bits) - 1   # INT_MAX / UINT64_MAX
        # (name, initial value or None for the default, call(addr, pe, init) -> returned old or None,
        #  final(init))
        arg = 0x0F0F00F0 + 7 * me
        cases = []
        if ty != "uint32":   # the AMO table's forms (uint32 stands for the bitwise 4-byte class only)
            cases += [
                ("compare_swap hit", None, lambda a, pe, i: fn("atomic_compare_swap")(a, w(i), w(arg), pe), lambda i: arg),
                ("compare_swap miss", None, lambda a, pe, i: fn("atomic_compare_swap")(a, w(i + 1), w(arg), pe), lambda i: i),
                ("fetch_inc", None, lambda a, pe, i: fn("atomic_fetch_inc")(a, pe), lambda i: i + 1),
                ("inc", None, lambda a, pe, i: fn("atomic_inc")(a, pe), lambda i: i + 1),
                ("fetch_add", None, lambda a, pe, i: fn("atomic_fetch_add")(a, w(arg), pe), lambda i: i + arg),
                ("add", None, lambda a, pe, i: fn("atomic_add")(a, w(-3), pe), lambda i: i - 3),
                # wrap-around: INT_MAX + 1, UINT64_MAX + 2
                ("fetch_add wraps", top, lambda a, pe, i: fn("atomic_fetch_add")(a, w(1 if signed else 2), pe),
                 lambda i: i + (1 if signed else 2)),
                ("fetch_inc wraps", top, lambda a, pe, i: fn("atomic_fetch_inc")(a, pe), lambda i: i + 1),
                ("swap", None, lambda a, pe, i: fn("atomic_swap")(a, w(arg), pe), lambda i: arg),
                ("fetch", None, lambda a, pe, i: fn("atomic_fetch")(a, pe), lambda i: i),
                ("set", None, lambda a, pe, i: fn("atomic_set")(a, w(arg), pe), lambda i: arg),
            ]
        if ty in ("uint32", "uint64"):
            cases += [
                ("and", None, lambda a, pe, i: fn("atomic_and")(a, w(arg), pe), lambda i: i & arg),
                ("or", None, lambda a, pe, i: fn("atomic_or")(a, w(arg), pe), lambda i: i | arg),
                ("xor", None, lambda a, pe, i: fn("atomic_xor")(a, w(arg), pe), lambda i: i ^ arg),
                ("fetch_and", None, lambda a, pe, i: fn("atomic_fetch_and")(a, w(arg), pe), lambda i: i & arg),
                ("fetch_or", None, lambda a, pe, i: fn("atomic_fetch_or")(a, w(arg), pe), lambda i: i | arg),
                ("fetch_xor", None, lambda a, pe, i: fn("atomic_fetch_xor")(a, w(arg), pe), lambda i: i ^ arg),
            ]
        if ty == "long":     # the deprecated aliases, once each
            cases += [
                ("cswap", None, lambda a, pe, i: fn("cswap")(a, w(i), w(arg), pe), lambda i: arg),
                ("finc", None, lambda a, pe, i: fn("finc")(a, pe), lambda i: i + 1),
                ("inc (old)", None, lambda a, pe, i: fn("inc")(a, pe), lambda i: i + 1),
                ("fadd", None, lambda a, pe, i: fn("fadd")(a, w(arg), pe), lambda i: i + arg),
                ("add (old)", None, lambda a, pe, i: fn("add")(a, w(arg), pe), lambda i: i + arg),
                ("swap (old)", None, lambda a, pe, i: fn("swap")(a, w(arg), pe), lambda i: arg),
                ("fetch (old)", None, lambda a, pe, i: fn("fetch")(a, pe), lambda i: i),
                ("set (old)", None, lambda a, pe, i: fn("set")(a, w(arg), pe), lambda i: arg),
            ]
        init = lambda owner, c, k: cases[c][1] if cases[c][1] is not None else init_of(owner, c, k, bits)  # noqa: E731
        for c in range(len(cases)):
            for k in range(3):
                put(slot(c, k), w(init(me, c, k)), me)
        S.shmem_barrier_all()
        for c, (name, _, call, final) in enumerate(cases):
            for k, pe in targets:
                old = call(slot(c, k), pe, init(pe, c, k))
                if old is not None:
                    expect(w(init(pe, c, k)), old, (ty, name, "old", "pe", pe))
        S.shmem_barrier_all()
        for c, (name, _, call, final) in enumerate(cases):
            for k, pe in targets:
                # the word on PE `pe` that this PE operated on, read back from there
                expect(w(final(init(pe, c, k))), get(slot(c, k), pe), (ty, name, "final", "pe", pe))
        S.shmem_barrier_all()

    # ---- float and double: set / fetch / swap on bit patterns ---------------------------------------
    for ty, bits in FLOATS.items():
        fn = lambda form: getattr(S, f"shmem_{ty}_{form}")  # noqa: E731
        put, get = getattr(S, f"shmem_{ty}_p"), getattr(S, f"shmem_{ty}_g")
        nan, neg0 = (NAN32, NEG0_32) if bits == 32 else (NAN64, NEG0_64)
        fb = lambda b: f_from_bits(b, bits)  # noqa: E731
        plain = f_bits(1.5 + me, bits)
        # (name, initial bits, call -> old float or None, final bits)
        cases = [("swap", f_bits(2.25, bits), lambda a, pe: fn("atomic_swap")(a, fb(plain), pe), plain),
                 ("swap in a NaN", f_bits(-7.0, bits), lambda a, pe: fn("atomic_swap")(a, fb(nan), pe), nan),
                 ("swap out a NaN", nan, lambda a, pe: fn("atomic_swap")(a, fb(neg0), pe), neg0),
                 ("swap out -0", neg0, lambda a, pe: fn("atomic_swap")(a, fb(plain), pe), plain),
                 ("fetch a NaN", nan, lambda a, pe: fn("atomic_fetch")(a, pe), nan),
                 ("fetch -0", neg0, lambda a, pe: fn("atomic_fetch")(a, pe), neg0),
                 ("set a NaN", f_bits(3.0, bits), lambda a, pe: fn("atomic_set")(a, fb(nan), pe), nan),
                 ("set -0", f_bits(3.0, bits), lambda a, pe: fn("atomic_set")(a, fb(neg0), pe), neg0)]
        for c, (name, init, _, _) in enumerate(cases):
            for k in range(3):
                put(slot(c, k), fb(init), me)
        S.shmem_barrier_all()
        for c, (name, init, call, final) in enumerate(cases):
            for k, pe in targets:
                old = call(slot(c, k), pe)
                if old is not None:
                    expect(hex(init), hex(f_bits(old, bits)), (ty, name, "old bits", "pe", pe))
        S.shmem_barrier_all()
        for c, (name, init, call, final) in enumerate(cases):
            for k, pe in targets:
                expect(hex(final), hex(f_bits(get(slot(c, k), pe), bits)), (ty, name, "final bits", "pe", pe))
            # and the bytes themselves, where they lie
            raw = R.device_bytes(slot(c, 0), bits // 8).tobytes()
            expect(hex(final), hex(int.from_bytes(raw, "little")), (ty, name, "own bytes"))
        S.shmem_barrier_all()

    # ---- contended fetch-add: every PE draws K tickets from PE 0's counter ---------------------------
    ctr = words
    S.shmem_long_p(ctr, 0, me)
    S.shmem_barrier_all()
    drawn = [S.shmem_long_atomic_fetch_add(ctr, 1, 0) for _ in range(K_CONTENDED)]
    arr = np.array(drawn, dtype=np.int64)
    L.check(L.lib().sosx_memcpy(mine, arr.ctypes.data, arr.nbytes, None), "sosx_memcpy")
    S.shmem_barrier_all()
    expect(P * K_CONTENDED, S.shmem_long_g(ctr, 0), "contended counter on PE 0")
    S.shmem_long_fcollect(world, gathered, mine, K_CONTENDED)
    allv = np.frombuffer(R.device_bytes(gathered, 8 * K_CONTENDED * P).tobytes(), np.int64)
    expect(list(range(P * K_CONTENDED)), sorted(allv.tolist()), "contended tickets: the union of all fetched values")
    expect(True, drawn == sorted(drawn), "contended tickets: each PE's own are increasing")
    S.shmem_barrier_all()

    # ---- non-fetching burst: no sync between the adds, one quiet ---------------------------------------
    x = words + 8
    S.shmem_int_p(x, 0, me)
    S.shmem_barrier_all()
    add = S.shmem_int_atomic_add
    for _ in range(K_BURST):
        add(x, me + 1, 0)
    S.shmem_quiet()
    S.shmem_barrier_all()
    expect(K_BURST * sum(pe + 1 for pe in range(P)), S.shmem_int_g(x, 0), "burst sum on PE 0")
    S.shmem_barrier_all()

    # ---- claim word: exactly one PE's compare-swap sees 0 -------------------------------------------
    claim, votes = words + 16, words + 8 * 128     # votes: P ints on every PE
    S.shmem_int_p(claim, 0, me)
    S.shmem_barrier_all()
    got = S.shmem_int_atomic_compare_swap(claim, 0, me + 1, 0)
    src = np.array([got], dtype=np.int32)
    L.check(L.lib().sosx_memcpy(mine, src.ctypes.data, 4, None), "sosx_memcpy")
    S.shmem_barrier_all()
    S.shmem_int_fcollect(world, votes, mine, 1)
    seen = np.frombuffer(R.device_bytes(votes, 4 * P).tobytes(), np.int32).tolist()
    winner = S.shmem_int_g(claim, 0)
    expect(1, seen.count(0), ("claim word: PEs that saw 0", seen))
    expect(True, 1 <= winner <= P and seen[winner - 1] == 0, ("claim word: the final word is the winner's", winner, seen))
    expect([winner] * (P - 1), [v for v in seen if v != 0], ("claim word: every other PE saw the winner", seen))
    S.shmem_barrier_all()

    # ---- nbi forms: fetch in device, pinned and pageable memory, more outstanding than the ring -----
    pinned = S.shmem_malloc(8 * N_NBI)
    for kind in ("device", "pinned", "pageable"):
        if kind == "device":
            t = torch.zeros(N_NBI, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            fptr = t.data_ptr()
        elif kind == "pinned":
            ctypes.memset(pinned, 0, 8 * N_NBI)
            fptr = pinned
        else:
            host = np.zeros(N_NBI, dtype=np.int64)
            fptr = host.ctypes.data

        def fetched(dtype):
            if kind == "device":
                raw = R.device_bytes(fptr, 8 * N_NBI).tobytes()
            elif kind == "pinned":
                raw = ctypes.string_at(pinned, 8 * N_NBI)
            else:
                raw = host.tobytes()
            return np.frombuffer(raw, dtype)

        # fetch_add_nbi: N outstanding on the right neighbour's one word, then ONE quiet
        w0 = words + 32
        S.shmem_long_p(w0, 1000 * (me + 1), me)
        S.shmem_barrier_all()
        for i in range(N_NBI):
            S.shmem_long_atomic_fetch_add_nbi(fptr + 8 * i, w0, 3, right)
        S.shmem_quiet()
        expect([1000 * (right + 1) + 3 * i for i in range(N_NBI)], fetched(np.int64).tolist(), ("fetch_add_nbi", kind))
        S.shmem_barrier_all()
        expect(1000 * (me + 1) + 3 * N_NBI, S.shmem_long_g(w0, me), ("fetch_add_nbi final", kind))
        # swap_nbi (double bit patterns), compare_swap_nbi, fetch_or_nbi: one each per target
        S.shmem_double_p(words + 40, f_from_bits(NAN64, 64), me)
        S.shmem_uint64_p(words + 48, 5 + me, me)
        S.shmem_uint32_p(words + 56, 0xF0 + me, me)
        S.shmem_barrier_all()
        S.shmem_double_atomic_swap_nbi(fptr, words + 40, f_from_bits(NEG0_64, 64), right)
        S.shmem_uint64_atomic_compare_swap_nbi(fptr + 8, words + 48, 5 + right, 77, right)
        S.shmem_uint32_atomic_fetch_or_nbi(fptr + 16, words + 56, 0x0F00, right)
        S.shmem_long_atomic_fetch_inc_nbi(fptr + 24, w0, right)
        S.shmem_quiet()
        f64 = fetched(np.uint64)
        expect(hex(NAN64), hex(int(f64[0])), ("swap_nbi old bits", kind))
        expect(5 + right, int(f64[1]), ("compare_swap_nbi old", kind))
        expect(0xF0 + right, int(fetched(np.uint32)[4]), ("fetch_or_nbi old", kind))
        expect(1000 * (right + 1) + 3 * N_NBI, int(fetched(np.int64)[3]), ("fetch_inc_nbi old", kind))
        S.shmem_barrier_all()
        expect(hex(NEG0_64), hex(f_bits(S.shmem_double_g(words + 40, me), 64)), ("swap_nbi final", kind))
        expect(77, S.shmem_uint64_g(words + 48, me), ("compare_swap_nbi final", kind))
        expect(0xFF0 + me, S.shmem_uint32_g(words + 56, me), ("fetch_or_nbi final", kind))
        S.shmem_barrier_all()

    # ---- the calling PE itself with the target on the HOST heap ------------------------------------
    # (static data, registered and pageable: tests/amo_static_pe.c)
    hw = pinned
    ctypes.memset(hw, 0, 64)
    ctypes.c_long.from_address(hw).value = 40
    expect(40, S.shmem_long_atomic_fetch_add(hw, 2, me), "host heap fetch_add old")
    S.shmem_long_atomic_inc(hw, me)
    S.shmem_quiet()
    expect(43, ctypes.c_long.from_address(hw).value, "host heap word after add and inc")
    expect(43, S.shmem_long_atomic_compare_swap(hw, 43, -1, me), "host heap compare_swap old")
    expect(-1, S.shmem_long_atomic_fetch(hw, me), "host heap fetch")
    ctypes.c_uint32.from_address(hw + 8).value = 0xFF00FF00
    S.shmem_uint32_atomic_xor(hw + 8, 0x0FF00FF0, me)
    S.shmem_quiet()
    expect(0xF0F0F0F0, ctypes.c_uint32.from_address(hw + 8).value, "host heap xor")
    expect(0, f_bits(S.shmem_float_atomic_swap(hw + 12, f_from_bits(NAN32, 32), me), 32), "host heap float swap old (+0)")
    expect(NAN32, ctypes.c_uint32.from_address(hw + 12).value, "host heap float swap bits")
    S.shmem_barrier_all()

    acq, reads, unacq = acquire_stats()
    if unacq:
        bad.append(("unacquired peer reads", unacq))
    S.shmem_barrier_all()
    S.shmem_free(pinned)
    for p in (mine, gathered, words):
        S.shmemx_free_device(p)
    sig = {1: "stream", 0: "host"}.get(L.lib().sosx_p2p_signal_mode(), "none")
    S.shmem_finalize()
    if bad:
        print(f"PE {me}/{P}: {len(bad)} of {checks} checks FAILED: {bad[:6]}", flush=True)
        return 1
    print(f"PE {me}/{P}: {checks} checks OK (p2p signal {sig}, peer reads {reads}, {unacq} unacquired)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
