"""Python mirror of the shmem.h reduction API (ctypes over libsos_amd.so).

Same names, argument meaning and error behaviour as SOS's C API
(src/collectives_c.c4:221-269): ``shmem_float_sum_reduce(team, dest, source, nreduce)``
returns 0, ``shmem_double_sum_to_all(target, source, nreduce, PE_start, logPE_stride,
PE_size, pWrk, pSync)`` returns None, and invalid arguments abort the process with an
SOS-style message.  Buffers are raw addresses (ints): device pointers (e.g. a torch
tensor's ``data_ptr()``) run in place on the GPU; host addresses are staged.
"""
import ctypes
import os
import re

from . import _lib

_c = ctypes
_RUNTIME = {
    "shmem_init": (None, []),
    "shmem_finalize": (None, []),
    "shmem_my_pe": (_c.c_int, []),
    "shmem_n_pes": (_c.c_int, []),
    "shmem_barrier_all": (None, []),
    "shmem_malloc": (_c.c_void_p, [_c.c_size_t]),
    "shmem_calloc": (_c.c_void_p, [_c.c_size_t, _c.c_size_t]),
    "shmem_free": (None, [_c.c_void_p]),
    "shmem_team_my_pe": (_c.c_int, [_c.c_void_p]),
    "shmem_team_n_pes": (_c.c_int, [_c.c_void_p]),
    "shmem_team_split_strided": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                            _c.c_long, _c.POINTER(_c.c_void_p)]),
    "shmem_team_destroy": (None, [_c.c_void_p]),
    "shmem_team_split_2d": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_long,
                                       _c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_long,
                                       _c.POINTER(_c.c_void_p)]),
    "shmem_team_translate_pe": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    "shmem_team_get_config": (_c.c_int, [_c.c_void_p, _c.c_long, _c.c_void_p]),
    "shmem_team_sync": (_c.c_int, [_c.c_void_p]),
    "shmemx_get_unique_id": (_c.c_int, [_c.c_void_p, _c.c_size_t]),
    "shmemx_init_attr": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t]),
    "shmemx_malloc_device": (_c.c_void_p, [_c.c_size_t]),
    "shmemx_free_device": (None, [_c.c_void_p]),
    "shmemx_set_stream": (None, [_c.c_void_p]),
    "shmemx_get_stream": (_c.c_void_p, []),
    "shmemx_set_reduce_algorithm": (_c.c_int, [_c.c_int]),
    "shmemx_set_transport": (_c.c_int, [_c.c_int]),
    "shmemx_get_device": (_c.c_int, []),
    "shmemx_reduce_local": (_c.c_int, [_c.c_int, _c.c_int, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "sosx_loopback_allreduce": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                           _c.c_size_t, _c.c_void_p]),
    "sosx_plan_encode": (_c.c_longlong, [_c.c_int, _c.c_int, _c.c_int, _c.c_ulonglong,
                                         _c.c_ulonglong, _c.c_uint, _c.c_uint,
                                         _c.POINTER(_c.c_longlong), _c.c_ulonglong]),
    "sosx_plan_encode_collect": (_c.c_longlong, [_c.c_int, _c.c_int, _c.POINTER(_c.c_ulonglong),
                                                 _c.POINTER(_c.c_ulonglong), _c.POINTER(_c.c_ulonglong),
                                                 _c.POINTER(_c.c_longlong), _c.c_ulonglong]),
    "sosx_loopback_collect": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                         _c.POINTER(_c.c_size_t), _c.c_void_p]),
    "sosx_resolve_alg": (_c.c_int, [_c.c_int, _c.c_ulonglong, _c.c_ulonglong]),
    "shmem_broadcastmem": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int]),
    "shmem_broadcast32": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                 _c.c_int, _c.c_void_p]),
    "shmem_broadcast64": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                 _c.c_int, _c.c_void_p]),
    "shmem_fcollectmem": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "shmem_alltoallmem": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "shmem_alltoallsmem": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_ssize_t,
                                      _c.c_ssize_t, _c.c_size_t]),
    "shmem_collectmem": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "shmem_collect32": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                               _c.c_void_p]),
    "shmem_collect64": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                               _c.c_void_p]),
    "shmem_fcollect32": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p]),
    "shmem_fcollect64": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p]),
    "shmem_alltoall32": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p]),
    "shmem_alltoall64": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p]),
    "shmem_alltoalls32": (None, [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t,
                                 _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "shmem_alltoalls64": (None, [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t,
                                 _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    # one-sided put / get: the generic entries behind the typed forms (rma.cpp), for the tests
    "shmem_quiet": (None, []),
    "shmem_fence": (None, []),
    "sos_api_put": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_int, _c.c_int, _c.c_char_p]),
    "sos_api_get": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_int, _c.c_int, _c.c_char_p]),
    "sos_api_iput": (None, [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t, _c.c_size_t,
                            _c.c_int, _c.c_char_p]),
    "sos_api_iget": (None, [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t, _c.c_size_t,
                            _c.c_int, _c.c_char_p]),
    "sos_api_ibput": (None, [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t, _c.c_size_t,
                             _c.c_size_t, _c.c_int, _c.c_char_p]),
    "sos_api_ibget": (None, [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t, _c.c_size_t,
                             _c.c_size_t, _c.c_int, _c.c_char_p]),
    "sos_api_p": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_char_p]),
    "sos_api_g": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_char_p]),
    "sos_api_ptr": (_c.c_void_p, [_c.c_void_p, _c.c_int]),
    "shmem_ptr": (_c.c_void_p, [_c.c_void_p, _c.c_int]),
    "sosx_block_strided_copy": (_c.c_int, [_c.c_void_p, _c.c_ssize_t, _c.c_void_p, _c.c_ssize_t, _c.c_size_t,
                                           _c.c_size_t, _c.c_size_t, _c.c_void_p]),
    "sosx_block_copy_plan": (_c.c_int, [_c.c_void_p, _c.c_ssize_t, _c.c_void_p, _c.c_ssize_t, _c.c_size_t,
                                        _c.c_size_t, _c.c_size_t, _c.POINTER(_c.c_longlong)]),
    # atomic memory operations: the generic entry, its checks and the kernel's C ABI (amo.cpp, onesided_checks.cpp, amo.hip)
    "sos_api_amo": (None, [_c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_size_t,
                           _c.c_int, _c.c_int, _c.c_int, _c.c_char_p]),
    "sos_amo_check": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "sosx_amo": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_size_t, _c.c_int,
                            _c.c_void_p]),
    # put with signal, signal operations, waits and tests: the generic entries, their checks, the
    # comparison and the kernels' C ABI (signal.cpp, onesided_checks.cpp, putsignal.hip)
    "sos_api_put_signal": (None, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_void_p, _c.c_uint64,
                                  _c.c_int, _c.c_int, _c.c_int, _c.c_char_p]),
    "sos_api_signal_op": (None, [_c.c_void_p, _c.c_uint64, _c.c_int, _c.c_int, _c.c_char_p]),
    "sos_api_signal_fetch": (_c.c_uint64, [_c.c_void_p, _c.c_char_p]),
    "sos_api_wait": (_c.c_size_t, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                   _c.c_int, _c.c_int, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_char_p]),
    "sos_api_test": (_c.c_size_t, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                   _c.c_int, _c.c_int, _c.c_size_t, _c.c_int, _c.c_char_p]),
    "sos_put_signal_check": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "sos_sync_check": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "sos_sync_eval": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                 _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "sosx_put_signal": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_uint64, _c.c_int,
                                   _c.c_void_p]),
    "sosx_put_signal_plan": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_longlong)]),
    "sosx_put_signal_ticket": (_c.c_void_p, []),
    "sosx_set_put_signal_fused_max": (_c.c_size_t, [_c.c_size_t]),
    "sosx_signal_stats": (None, [_c.POINTER(_c.c_long), _c.POINTER(_c.c_long), _c.POINTER(_c.c_long)]),
    "sosx_sync_snapshot": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_size_t, _c.c_void_p]),
    "shmem_signal_fetch": (_c.c_uint64, [_c.c_void_p]),
    "shmemx_signal_add": (None, [_c.c_void_p, _c.c_uint64, _c.c_int]),
    "shmemx_signal_set": (None, [_c.c_void_p, _c.c_uint64, _c.c_int]),
    "shmem_signal_wait_until": (_c.c_uint64, [_c.c_void_p, _c.c_int, _c.c_uint64]),
    "shmem_wait": (None, [_c.c_void_p, _c.c_long]),
    "shmem_wait_until": (None, [_c.c_void_p, _c.c_int, _c.c_long]),
    # distributed locks: the three names, the generic entries, the check and message functions and the
    # kernel's C ABI (lock.cpp, onesided_checks.cpp, lock.hip)
    "shmem_set_lock": (None, [_c.c_void_p]),
    "shmem_clear_lock": (None, [_c.c_void_p]),
    "shmem_test_lock": (_c.c_int, [_c.c_void_p]),
    "sos_api_set_lock": (None, [_c.c_void_p, _c.c_char_p]),
    "sos_api_clear_lock": (None, [_c.c_void_p, _c.c_char_p]),
    "sos_api_test_lock": (_c.c_int, [_c.c_void_p, _c.c_char_p]),
    "sos_lock_check": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "sos_lock_expiry_message": (None, [_c.c_char_p, _c.c_void_p, _c.c_int, _c.c_uint32, _c.c_double, _c.c_char_p,
                                       _c.c_size_t]),
    "sos_lock_corrupt_message": (None, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_char_p, _c.c_size_t]),
    "sosx_lock_step": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_int,
                                  _c.c_void_p, _c.c_void_p]),
    "sosx_lock_table": (_c.c_void_p, [_c.POINTER(_c.c_int)]),
    "sosx_lock_stats": (None, [_c.POINTER(_c.c_long), _c.POINTER(_c.c_long)]),
    # communication contexts: the checks and the pool's size (ctx.cpp, onesided_checks.cpp); the public
    # names are _CTX_RUNTIME's and __getattr__'s, from libsos_amd_ctx.so
    "sos_ctx_check": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.c_char_p,
                                 _c.c_size_t]),
    "sos_ctx_options_check": (_c.c_int, [_c.c_long, _c.c_char_p, _c.c_size_t]),
    "sos_ctx_pool_size": (_c.c_int, [_c.c_char_p, _c.c_char_p, _c.c_size_t]),
    "sos_ctx_stream_slot": (_c.c_int, [_c.c_ulong, _c.c_int]),
    "sosx_ctx_streams": (_c.c_int, []),
    "sosx_put_signal_on": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_uint64, _c.c_int,
                                      _c.c_void_p, _c.c_void_p]),
    "sosx_prof_enable": (None, [_c.c_int]),
    "sosx_prof_get": (None, [_c.POINTER(_c.c_double), _c.POINTER(_c.c_double),
                             _c.POINTER(_c.c_long), _c.POINTER(_c.c_long), _c.POINTER(_c.c_long)]),
}

# the context management calls (libsos_amd_ctx.so); the ctx twins of the typed calls resolve in __getattr__
_CTX_RUNTIME = {
    "shmem_ctx_create": (_c.c_int, [_c.c_long, _c.POINTER(_c.c_void_p)]),
    "shmem_ctx_destroy": (None, [_c.c_void_p]),
    "shmem_ctx_quiet": (None, [_c.c_void_p]),
    "shmem_ctx_fence": (None, [_c.c_void_p]),
    "shmem_team_create_ctx": (_c.c_int, [_c.c_void_p, _c.c_long, _c.POINTER(_c.c_void_p)]),
    "shmem_ctx_get_team": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_void_p)]),
}

_REDUCE_RE = re.compile(r"^shmem_(\w+?)_(and|or|xor|min|max|sum|prod)_(reduce|to_all)$")
_SCAN_RE = re.compile(r"^shmemx_(\w+?)_sum_(inscan|exscan)$")
_BCAST_RE = re.compile(r"^shmem_(\w+?)_broadcast$")
_COLLECT_RE = re.compile(r"^shmem_(\w+?)_(fcollect|alltoalls|alltoall|collect)$")
# shmem_<T>_put / get / put_nbi / get_nbi / iput / iget / p / g, shmem_put<N> ..., putmem / getmem,
# shmemx_<T>_ibput / ibget and shmemx_ibput<N> / ibget<N>
_RMA_RE = re.compile(r"^shmemx?_(?:(\w+?)_)?(ibput|ibget|iput|iget|put|get|p|g)(\d+|mem)?(_nbi)?$")
# shmem_<T>_atomic_<op>[_nbi] and the deprecated shmem_<T>_<cswap|finc|inc|fadd|add|swap|fetch|set>
_AMO_RE = re.compile(r"^shmem_(\w+?)_(?:atomic_(compare_swap|fetch_inc|inc|fetch_add|add|swap|fetch|set|and|or|xor|"
                     r"fetch_and|fetch_or|fetch_xor)(_nbi)?|(cswap|finc|inc|fadd|add|swap|fetch|set))$")
_AMO_OLD = {"cswap": "compare_swap", "finc": "fetch_inc", "fadd": "fetch_add"}
_AMO_TYPES = ("int", "long", "longlong", "uint", "ulong", "ulonglong", "int32", "int64", "uint32", "uint64",
              "size", "ptrdiff", "float", "double")
# shmem_<T>_put_signal[_nbi], shmem_put<N>_signal[_nbi], shmem_putmem_signal[_nbi]
_PUT_SIGNAL_RE = re.compile(r"^shmem_(?:(\w+?)_put|put(?:\d+|mem))_signal(_nbi)?$")
# shmem_<T>_wait_until / _test with their _all / _any / _some and _vector forms, and the deprecated shmem_<T>_wait
_SYNC_RE = re.compile(r"^shmem_(\w+?)_(?:(wait_until|test)(?:_(all|any|some))?(_vector)?|(wait))$")
_SYNC_TYPES = ("short", "int", "long", "longlong", "ushort", "uint", "ulong", "ulonglong", "int32", "int64",
               "uint32", "uint64", "size", "ptrdiff")
_BY_VALUE = {"char": _c.c_char, "schar": _c.c_byte, "short": _c.c_short, "int": _c.c_int, "long": _c.c_long,
             "longlong": _c.c_longlong, "uchar": _c.c_ubyte, "ushort": _c.c_ushort, "uint": _c.c_uint,
             "ulong": _c.c_ulong, "ulonglong": _c.c_ulonglong, "int8": _c.c_int8, "int16": _c.c_int16,
             "int32": _c.c_int32, "int64": _c.c_int64, "uint8": _c.c_uint8, "uint16": _c.c_uint16,
             "uint32": _c.c_uint32, "uint64": _c.c_uint64, "size": _c.c_size_t, "ptrdiff": _c.c_ssize_t,
             "float": _c.c_float, "double": _c.c_double, "longdouble": _c.c_longdouble}
# the ctx twin of a typed call: shmem_ctx_<rest> / shmemx_ctx_<rest>, its plain form's arguments
# behind a leading context handle
_CTX_RE = re.compile(r"^(shmemx?)_ctx_(\w+)$")
SHMEM_CTX_PRIVATE, SHMEM_CTX_SERIALIZED, SHMEM_CTX_NOSTORE = 1, 2, 4
_declared = False
_CTX_LIB = None


def lib():
    global _declared
    L = _lib.lib()
    if not _declared:
        for name, (res, args) in _RUNTIME.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _declared = True
    return L


def ctx_lib():
    """libsos_amd_ctx.so: the public shmem_ctx_* names.  It binds to whichever build of the
    runtime lib() loaded (globally) before it."""
    global _CTX_LIB
    if _CTX_LIB is None:
        lib()
        _CTX_LIB = ctypes.CDLL(os.path.join(_lib.HERE, "libsos_amd_ctx.so"))
    return _CTX_LIB


def team_world():
    return ctypes.c_void_p.in_dll(lib(), "SHMEM_TEAM_WORLD").value


def team_shared():
    return ctypes.c_void_p.in_dll(lib(), "SHMEM_TEAM_SHARED").value


def ctx_default():
    return ctypes.c_void_p.in_dll(lib(), "SHMEM_CTX_DEFAULT").value


def team_node():
    return ctypes.c_void_p.in_dll(lib(), "SHMEMX_TEAM_NODE").value


def __getattr__(name):
    """shmem_<T>_<op>_reduce / _to_all, shmem_init, ... resolved from the library."""
    L = lib()
    m = _REDUCE_RE.match(name)
    if m:
        fn = getattr(L, name)
        if m.group(3) == "reduce":
            fn.restype = ctypes.c_int
            fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]
        else:
            fn.restype = None
            fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                           _c.c_void_p, _c.c_void_p]
        return fn
    if _SCAN_RE.match(name):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t]
        return fn
    if _BCAST_RE.match(name):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int]
        return fn
    m = _COLLECT_RE.match(name)
    if m and name not in _RUNTIME:
        # shmem_<T>_fcollect / _alltoall / _collect (team, dest, source, nelems) and
        # shmem_<T>_alltoalls (team, dest, source, dst, sst, nelems)
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        strides = [_c.c_ssize_t, _c.c_ssize_t] if m.group(2) == "alltoalls" else []
        fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_void_p] + strides + [_c.c_size_t]
        return fn
    if name in _RUNTIME:
        return getattr(L, name)
    if name in _CTX_RUNTIME:
        fn = getattr(ctx_lib(), name)
        fn.restype, fn.argtypes = _CTX_RUNTIME[name]
        return fn
    m = _CTX_RE.match(name)
    if m:
        fn = getattr(ctx_lib(), name)  # AttributeError where SOS has no ctx form (locks, waits, deprecated atomics)
        plain = __getattr__(f"{m.group(1)}_{m.group(2)}")
        fn.restype = plain.restype
        fn.argtypes = [_c.c_void_p] + list(plain.argtypes)
        return fn
    m = _PUT_SIGNAL_RE.match(name)
    if m and (m.group(1) is None or m.group(1) in _BY_VALUE):
        # (target, source, nelems, sig_addr, signal, sig_op, pe)
        fn = getattr(L, name)
        fn.restype = None
        fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_int]
        return fn
    m = _SYNC_RE.match(name)
    if m and m.group(1) in _SYNC_TYPES:
        # the value by value, the _vector forms' values by address; _any / _some return a size_t,
        # test and test_all an int, the waits nothing
        ty = _BY_VALUE[m.group(1)]
        fn = getattr(L, name)
        if m.group(5):  # shmem_<T>_wait(var, value)
            fn.restype, fn.argtypes = None, [_c.c_void_p, ty]
            return fn
        what, kind, vector = m.group(2), m.group(3), bool(m.group(4))
        if kind is None:
            if vector:
                raise AttributeError(name)
            fn.restype = _c.c_int if what == "test" else None
            fn.argtypes = [_c.c_void_p, _c.c_int, ty]
            return fn
        fn.restype = _c.c_size_t if kind in ("any", "some") else (_c.c_int if what == "test" else None)
        fn.argtypes = ([_c.c_void_p, _c.c_size_t] + ([_c.c_void_p] if kind == "some" else [])
                       + [_c.c_void_p, _c.c_int, _c.c_void_p if vector else ty])
        return fn
    m = _AMO_RE.match(name)
    if m and m.group(1) in _AMO_TYPES:
        # values by value (float and double included); the nbi forms take `fetch` first and
        # return nothing; the fetching forms return the old value
        ty = _BY_VALUE[m.group(1)]
        form = m.group(2) or _AMO_OLD.get(m.group(4), m.group(4))
        nbi = bool(m.group(3))
        fn = getattr(L, name)
        operands = {"compare_swap": [ty, ty], "fetch_inc": [], "inc": [], "fetch": []}.get(form, [ty])
        fetching = form in ("compare_swap", "swap", "fetch") or form.startswith("fetch_")
        fn.restype = ty if fetching and not nbi else None
        fn.argtypes = ([_c.c_void_p] if nbi else []) + [_c.c_void_p] + operands + [_c.c_int]
        return fn
    m = _RMA_RE.match(name)
    if m and (m.group(1) is None or m.group(1) in _BY_VALUE):
        ty, kind = m.group(1), m.group(2)
        fn = getattr(L, name)
        fn.restype = None
        if kind == "p":
            fn.argtypes = [_c.c_void_p, _BY_VALUE[ty], _c.c_int]
        elif kind == "g":
            fn.restype = _BY_VALUE[ty]
            fn.argtypes = [_c.c_void_p, _c.c_int]
        elif kind in ("put", "get"):
            fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int]
        elif kind in ("iput", "iget"):
            fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t, _c.c_int]
        else:
            fn.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_ssize_t, _c.c_ssize_t, _c.c_size_t, _c.c_size_t,
                           _c.c_int]
        return fn
    raise AttributeError(name)


def init_attr(rank, n_pes, uid):
    buf = ctypes.create_string_buffer(bytes(uid), 128)
    return _lib.check(lib().shmemx_init_attr(rank, n_pes, buf, 128), "shmemx_init_attr")


def get_unique_id():
    buf = ctypes.create_string_buffer(128)
    _lib.check(lib().shmemx_get_unique_id(buf, 128), "shmemx_get_unique_id")
    return buf.raw


def loopback_allreduce(alg, op, dtype, srcs, dsts, count, stream=None):
    P = len(srcs)
    s = (ctypes.c_void_p * P)(*srcs)
    d = (ctypes.c_void_p * P)(*dsts)
    a = _lib.ALGS[alg] if isinstance(alg, str) else int(alg)
    return _lib.check(lib().sosx_loopback_allreduce(a, P, _lib.op_id(op), _lib.dtype_id(dtype), s,
                                                    d, count, stream), "sosx_loopback_allreduce")


def plan(alg, P, me, count, ts, src_mis=0, dst_mis=0):
    """Decode the per-PE plan (see sos_amd/csrc/plan.cpp, sosx_plan_encode)."""
    a = _lib.ALGS[alg] if isinstance(alg, str) else int(alg)
    L = lib()
    n = L.sosx_plan_encode(a, P, me, count, ts, src_mis, dst_mis, None, 0)
    if n < 0:
        raise _lib.SosError(int(n), "sosx_plan_encode")
    buf = (ctypes.c_longlong * n)()
    L.sosx_plan_encode(a, P, me, count, ts, src_mis, dst_mis, buf, n)
    return _decode_plan(list(buf))


def plan_collect(P, me, lens):
    """The collect plan of PE `me` for the per-PE byte lengths `lens`
    (sosx_plan_encode_collect), with its "src_bytes" and "dst_bytes"."""
    L = lib()
    arr = (ctypes.c_ulonglong * max(len(lens), 1))(*lens)
    sb, db = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    n = L.sosx_plan_encode_collect(P, me, arr, ctypes.byref(sb), ctypes.byref(db), None, 0)
    if n < 0:
        raise _lib.SosError(int(n), "sosx_plan_encode_collect")
    buf = (ctypes.c_longlong * n)()
    L.sosx_plan_encode_collect(P, me, arr, None, None, buf, n)
    out = _decode_plan(list(buf))
    out.update(src_bytes=sb.value, dst_bytes=db.value)
    return out


def loopback_collect(srcs, dsts, lens, stream=None):
    """All P collect plans on one GPU (sosx_loopback_collect); lens in bytes."""
    P = len(lens)
    s = (ctypes.c_void_p * P)(*srcs)
    d = (ctypes.c_void_p * P)(*dsts)
    n = (ctypes.c_size_t * P)(*lens)
    return _lib.check(lib().sosx_loopback_collect(P, s, d, n, stream), "sosx_loopback_collect")


def _decode_plan(w):
    pos = 3
    rounds = []
    for _ in range(w[1]):
        nx, nops = w[pos], w[pos + 1]
        pos += 2
        xfers = []
        for _ in range(nx):
            send, peer, b, off, nbytes = w[pos:pos + 5]
            pos += 5
            xfers.append({"send": send, "peer": peer, "buf": b, "off": off, "bytes": nbytes})
        ops = []
        for _ in range(nops):
            kind, order, ob, ooff, nin, cnt = w[pos:pos + 6]
            pos += 6
            ins = []
            for _ in range(nin):
                ins.append((w[pos], w[pos + 1]))
                pos += 2
            nout = w[pos]
            pos += 1
            outs = []
            for _ in range(nout):
                outs.append((w[pos], w[pos + 1]))
                pos += 2
            ops.append({"kind": kind, "order": order, "out": (ob, ooff), "ins": ins, "count": cnt,
                        "outs": outs})
        rounds.append({"xfers": xfers, "ops": ops})
    return {"alg": w[0], "scratch_bytes": w[2], "rounds": rounds}


def prof_enable(on=True):
    lib().sosx_prof_enable(1 if on else 0)


def prof_get():
    f, x = ctypes.c_double(), ctypes.c_double()
    nf, nx, nc = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    lib().sosx_prof_get(ctypes.byref(f), ctypes.byref(x), ctypes.byref(nf), ctypes.byref(nx),
                        ctypes.byref(nc))
    return {"fold_ms": f.value, "xfer_ms": x.value, "nfold": nf.value, "nxfer": nx.value,
            "ncall": nc.value}
