#!/usr/bin/env python3
"""Generate the typed SOS reduction / scan / broadcast entry points.

SOS stamps its reductions out of m4 type tables (bindings/shmem_bind_c.m4:93-180)
through SHMEM_DEF_TO_ALL / SHMEM_DEF_REDUCE (src/collectives_c.c4:221-292).  This
generator holds the same tables -- including SOS's mapping of uint8/16/32/64 onto the
SIGNED INT8..INT64 internal types (shmem_bind_c.m4:113-116, :136-139, :162-165), which
makes their min/max compare signed -- and writes:

  include/shmem_reductions.h      198 prototypes + C11 _Generic macros
                                  (mpp/shmem.h4:952-991) + C++ overloads (:249-296)
  include/shmemx_scans.h          52 shmemx_<T>_sum_{inscan,exscan} prototypes + generics
                                  (mpp/shmemx_c_func.h4:78-86, mpp/shmemx.h4:71-133)
  sos_amd/csrc/reductions_gen.cpp the definitions (strong pshmem_*, weak shmem_*
                                  aliases as SOS's profiling interface,
                                  src/collectives_c.c4:36-166), plus the 24 typed team
                                  broadcasts shmem_<T>_broadcast (SHMEM_BIND_C_RMA,
                                  src/collectives_c.c4:402-429) and the 52 scans
                                  (src/collectives_c.c4:294-340)

  include/shmem_collects.h        72 shmem_<T>_{fcollect,alltoall,alltoalls} prototypes, the
                                  mem and active-set forms, generics and overloads
  sos_amd/csrc/collects_gen.cpp   their definitions (src/collectives_c.c4:536-707)

  include/shmem_collectv.h        24 shmem_<T>_collect prototypes, shmem_collectmem, the
                                  active-set shmem_collect32/64, generics and overloads
  sos_amd/csrc/collectv_gen.cpp   their definitions (src/collectives_c.c4:432-503)

  include/shmem_rma.h             the one-sided family: shmem_<T>_{put,get,put_nbi,get_nbi,p,g,
                                  iput,iget}, the sized and mem forms, shmem_ptr, generics and
                                  overloads (mpp/shmem_c_func.h4:46-241)
  include/shmemx_rma.h            shmemx_<T>_{ibput,ibget} and shmemx_{ibput,ibget}<N>
                                  (mpp/shmemx_c_func.h4:32-71)
  sos_amd/csrc/rma_gen.cpp        their definitions (src/data_c.c4:300-680) over rma.cpp

  include/shmem_amo.h             the atomic memory operations shmem_<T>_atomic_*, their
                                  deprecated names and nbi forms, generics and overloads
                                  (mpp/shmem_c_func.h4:243-404, :575-639)
  sos_amd/csrc/amo_gen.cpp        their definitions (src/atomic_c.c4) over amo.cpp

  include/shmem_signal.h          put with signal shmem_<T>_put_signal[_nbi], the sized and mem forms,
                                  shmem_signal_fetch, shmemx_signal_add / _set, generics and
                                  overloads (mpp/shmem_c_func.h4:91-127, mpp/shmemx_c_func.h4:98-100)
  include/shmem_sync.h            shmem_<T>_wait_until / _test with their _all / _any / _some and
                                  _vector forms, shmem_signal_wait_until, the deprecated waits
                                  (mpp/shmem_c_func.h4:473-542)
  sos_amd/csrc/signal_gen.cpp     their definitions (src/data_c.c4:684-784,
                                  src/synchronization_c.c4) over signal.cpp

  include/shmem_ctx.h             the communication contexts: shmem_ctx_create / destroy / quiet / fence,
                                  shmem_team_create_ctx, shmem_ctx_get_team and the shmem_ctx_ twin of
                                  every put, get, atomic and put with signal; redefines the generics to
                                  take a leading shmem_ctx_t (mpp/shmem_c_func.h4, mpp/shmem.h4)
  include/shmemx_ctx.h            shmemx_ctx_<T>_{ibput,ibget}, shmemx_ctx_ib{put,get}<N>,
                                  shmemx_ctx_signal_add / _set
  sos_amd/csrc/ctx_gen.cpp        their definitions over the sos_api_ctx_* entries

The library's Makefile compiles every *.cpp of the directory, so a new generated source
needs no entry there.

Run: python sos_amd/csrc/gen_bindings.py  (build() runs it; output is committed).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (stype, C type, internal datatype) -- bindings/shmem_bind_c.m4
COLL_INTS = [("short", "short", "SHORT"), ("int", "int", "INT"), ("long", "long", "LONG"),
             ("longlong", "long long", "LONG_LONG")]
AND_OR_XOR = [
    ("uchar", "unsigned char", "UCHAR"), ("short", "short", "SHORT"),
    ("ushort", "unsigned short", "USHORT"), ("int", "int", "INT"), ("uint", "unsigned int", "UINT"),
    ("long", "long", "LONG"), ("ulong", "unsigned long", "ULONG"),
    ("longlong", "long long", "LONG_LONG"), ("ulonglong", "unsigned long long", "ULONG_LONG"),
    ("int8", "int8_t", "INT8"), ("int16", "int16_t", "INT16"), ("int32", "int32_t", "INT32"),
    ("int64", "int64_t", "INT64"),
    ("uint8", "uint8_t", "INT8"), ("uint16", "uint16_t", "INT16"),    # signed ITYPE (SOS quirk)
    ("uint32", "uint32_t", "INT32"), ("uint64", "uint64_t", "INT64"),  # signed ITYPE (SOS quirk)
    ("size", "size_t", "SIZE_T")]
MIN_MAX = [
    ("char", "char", "CHAR"), ("schar", "signed char", "SCHAR"), ("short", "short", "SHORT"),
    ("int", "int", "INT"), ("long", "long", "LONG"), ("longlong", "long long", "LONG_LONG"),
    ("ptrdiff", "ptrdiff_t", "PTRDIFF_T"), ("uchar", "unsigned char", "UCHAR"),
    ("ushort", "unsigned short", "USHORT"), ("uint", "unsigned int", "UINT"),
    ("ulong", "unsigned long", "ULONG"), ("ulonglong", "unsigned long long", "ULONG_LONG"),
    ("int8", "int8_t", "INT8"), ("int16", "int16_t", "INT16"), ("int32", "int32_t", "INT32"),
    ("int64", "int64_t", "INT64"),
    ("uint8", "uint8_t", "INT8"), ("uint16", "uint16_t", "INT16"),
    ("uint32", "uint32_t", "INT32"), ("uint64", "uint64_t", "INT64"),
    ("size", "size_t", "SIZE_T"), ("float", "float", "FLOAT"), ("double", "double", "DOUBLE"),
    ("longdouble", "long double", "LONG_DOUBLE")]
SUM_PROD = MIN_MAX + [("complexd", "double _Complex", "DOUBLE_COMPLEX"),
                      ("complexf", "float _Complex", "FLOAT_COMPLEX")]
# bindings/shmem_bind_c.m4:10-34 (broadcast element types; bytes only, no ITYPE)
RMA = [("float", "float"), ("double", "double"), ("longdouble", "long double"), ("char", "char"),
       ("schar", "signed char"), ("short", "short"), ("int", "int"), ("long", "long"),
       ("longlong", "long long"), ("uchar", "unsigned char"), ("ushort", "unsigned short"),
       ("uint", "unsigned int"), ("ulong", "unsigned long"), ("ulonglong", "unsigned long long"),
       ("int8", "int8_t"), ("int16", "int16_t"), ("int32", "int32_t"), ("int64", "int64_t"),
       ("uint8", "uint8_t"), ("uint16", "uint16_t"), ("uint32", "uint32_t"), ("uint64", "uint64_t"),
       ("size", "size_t"), ("ptrdiff", "ptrdiff_t")]
# bindings/shmem_bind_c11.m4:13-28 (generic selector: base types only)
GENERIC_RMA = RMA[:14]
FLOATS = [("float", "float", "FLOAT"), ("double", "double", "DOUBLE"),
          ("longdouble", "long double", "LONG_DOUBLE")]
CMPLX = [("complexf", "float _Complex", "FLOAT_COMPLEX"),
         ("complexd", "double _Complex", "DOUBLE_COMPLEX")]

OPS = {"and": "BAND", "or": "BOR", "xor": "BXOR", "min": "MIN", "max": "MAX", "sum": "SUM",
       "prod": "PROD"}

# src/collectives_c.c4:270-292
TO_ALL = ([(t, o) for o in ("and", "or", "xor") for t in COLL_INTS]
          + [(t, "min") for t in COLL_INTS] + [(t, "min") for t in FLOATS]
          + [(t, "max") for t in COLL_INTS] + [(t, "max") for t in FLOATS]
          + [(t, "sum") for t in COLL_INTS] + [(t, "sum") for t in FLOATS] + [(t, "sum") for t in CMPLX]
          + [(t, "prod") for t in COLL_INTS] + [(t, "prod") for t in FLOATS] + [(t, "prod") for t in CMPLX])
REDUCE = ([(t, o) for o in ("and", "or", "xor") for t in AND_OR_XOR]
          + [(t, o) for o in ("sum", "prod") for t in SUM_PROD]
          + [(t, o) for o in ("min", "max") for t in MIN_MAX])

REDUCE_TABLE = {"and": AND_OR_XOR, "or": AND_OR_XOR, "xor": AND_OR_XOR, "min": MIN_MAX,
                "max": MIN_MAX, "sum": SUM_PROD, "prod": SUM_PROD}

# Generic (C11 _Generic / C++ overload) selector tables: base C types only
# (bindings/shmem_bind_c11.m4:69-112, bindings/shmem_bind_cxx.m4:63-107).  The
# fixed-width "extras" SOS appends at configure time are aliases of these base types
# on x86-64 glibc (int8_t = signed char, int64_t = long, size_t = unsigned long, ...),
# so none is distinct here.
_BASE_UNSIGNED = [("uchar", "unsigned char"), ("ushort", "unsigned short"),
                  ("uint", "unsigned int"), ("ulong", "unsigned long"),
                  ("ulonglong", "unsigned long long")]
_BASE_MIN_MAX = [("char", "char"), ("schar", "signed char"), ("short", "short"), ("int", "int"),
                 ("long", "long"), ("longlong", "long long")] + _BASE_UNSIGNED + [
                 ("float", "float"), ("double", "double"), ("longdouble", "long double")]
GENERIC_TABLE = {"and": _BASE_UNSIGNED, "or": _BASE_UNSIGNED, "xor": _BASE_UNSIGNED,
                 "min": _BASE_MIN_MAX, "max": _BASE_MIN_MAX,
                 "sum": _BASE_MIN_MAX + [("complexd", "double _Complex"),
                                         ("complexf", "float _Complex")]}
GENERIC_TABLE["prod"] = GENERIC_TABLE["sum"]


def to_all_sig(prefix, st, ct, op):
    return (f"void {prefix}shmem_{st}_{op}_to_all({ct} *target, const {ct} *source, int nreduce, "
            f"int PE_start, int logPE_stride, int PE_size, {ct} *pWrk, long *pSync)")


def reduce_sig(prefix, st, ct, op):
    return (f"int {prefix}shmem_{st}_{op}_reduce(shmem_team_t team, {ct} *dest, const {ct} *source, "
            f"size_t nreduce)")


def bcast_sig(prefix, st, ct):
    return (f"int {prefix}shmem_{st}_broadcast(shmem_team_t team, {ct} *dest, const {ct} *source, "
            f"size_t nelems, int PE_root)")


def scan_sig(prefix, st, ct, kind):
    return (f"int {prefix}shmemx_{st}_sum_{kind}(shmem_team_t team, {ct} *dest, const {ct} *source, "
            f"size_t nelems)")


SCANS = [(t, k) for k in ("exscan", "inscan") for t in SUM_PROD]


def c11_generic(name, arms, argidx=1):
    out = [f"#define {name}(...) \\",
           f"    _Generic(SHMEM_C11_TYPE_EVAL_PTR(SHMEM_C11_ARG{argidx}(__VA_ARGS__)), \\",
           ", \\\n".join(arms) + " \\", "    )(__VA_ARGS__)"]
    return out


def c11_prelude(guarded=True):
    """The helper macros of the C11 selectors.  shmem_reductions.h defines them
    unconditionally; the headers that may come after it guard them."""
    out = ["#define SHMEM_C11_TYPE_EVAL_PTR(arg) &*(arg)",
           "#define SHMEM_C11_ARG1(first, ...) SHMEM_C11_ARG1_HELPER(__VA_ARGS__, sentinel)",
           "#define SHMEM_C11_ARG1_HELPER(second, ...) second"]
    return ["#ifndef SHMEM_C11_TYPE_EVAL_PTR"] + out + ["#endif"] if guarded else out


def definition(out, sig, name, body):
    """One entry point: the strong pshmem form with its one-line body, the weak alias."""
    out += [sig("p"), "{", f"    {body}", "}", f"{sig('')} __attribute__((weak, alias(\"p{name}\")));", ""]


def scan_header():
    out = ["/* shmemx_scans.h -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.",
           " *",
           " * SOS's team prefix-sum extensions shmemx_<T>_sum_{inscan,exscan}",
           " * (mpp/shmemx_c_func.h4:78-86) with their C++ overloads and C11 generic",
           " * selectors (mpp/shmemx.h4:71-133). */",
           "#ifndef SHMEMX_SCANS_H", "#define SHMEMX_SCANS_H", "",
           "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    for (st, ct, it), k in SCANS:
        out.append(f"SHMEM_FUNCTION_ATTRIBUTES {scan_sig('', st, ct, k)};")
    for (st, ct, it), k in SCANS:
        out.append(f"{scan_sig('p', st, ct, k)};")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    out.append("#if defined(__cplusplus)")
    for k in ("exscan", "inscan"):
        for st, ct in GENERIC_TABLE["sum"]:
            out.append(f"static inline int shmemx_sum_{k}(shmem_team_t team, {ct} *dest, "
                       f"const {ct} *source, size_t nelems) {{ return shmemx_{st}_sum_{k}(team, "
                       f"dest, source, nelems); }}")
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    out += c11_prelude()
    for k in ("exscan", "inscan"):
        out += c11_generic(f"shmemx_sum_{k}",
                           [f"        {ct}*: shmemx_{st}_sum_{k}" for st, ct in GENERIC_TABLE["sum"]])
    out.append("#endif")
    out += ["", "#endif /* SHMEMX_SCANS_H */", ""]
    return "\n".join(out)


def header():
    out = ["/* shmem_reductions.h -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.",
           " *",
           " * The SOS reduction family: 44 active-set *_to_all and 154 team *_reduce entry",
           " * points with SOS's signatures (mpp/shmem_c_func.h4:413-438, :688-702), the 24",
           " * typed team broadcasts (:673-676), the C11 generic selectors (mpp/shmem.h4:",
           " * 934-939, :952-991) and C++ overloads (:228-233, :249-296). */",
           "#ifndef SHMEM_REDUCTIONS_H", "#define SHMEM_REDUCTIONS_H", "",
           "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    out.append("/* active-set reductions (deprecated in OpenSHMEM 1.5, kept by SOS) */")
    for (st, ct, it), op in TO_ALL:
        out.append(f"SHMEM_FUNCTION_ATTRIBUTES {to_all_sig('', st, ct, op)};")
    out.append("")
    out.append("/* team reductions */")
    for (st, ct, it), op in REDUCE:
        out.append(f"SHMEM_FUNCTION_ATTRIBUTES {reduce_sig('', st, ct, op)};")
    out.append("")
    out.append("/* typed team broadcasts (mpp/shmem_c_func.h4:673-676) */")
    for st, ct in RMA:
        out.append(f"SHMEM_FUNCTION_ATTRIBUTES {bcast_sig('', st, ct)};")
    out.append("")
    out.append("/* profiling interface: pshmem_* are the implementations, shmem_* weak aliases */")
    for (st, ct, it), op in TO_ALL:
        out.append(f"{to_all_sig('p', st, ct, op)};")
    for (st, ct, it), op in REDUCE:
        out.append(f"{reduce_sig('p', st, ct, op)};")
    for st, ct in RMA:
        out.append(f"{bcast_sig('p', st, ct)};")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    # C++ overloads
    out.append("#if defined(__cplusplus)")
    for op in ("and", "or", "xor", "min", "max", "sum", "prod"):
        for st, ct in GENERIC_TABLE[op]:
            out.append(f"static inline int shmem_{op}_reduce(shmem_team_t team, {ct} *dest, "
                       f"const {ct} *source, size_t nreduce) {{ return shmem_{st}_{op}_reduce(team, "
                       f"dest, source, nreduce); }}")
    for st, ct in GENERIC_RMA:
        out.append(f"static inline int shmem_broadcast(shmem_team_t team, {ct} *dest, const {ct} *source, "
                   f"size_t nelems, int PE_root) {{ return shmem_{st}_broadcast(team, dest, source, "
                   f"nelems, PE_root); }}")
    # C11 generics
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    out += c11_prelude(guarded=False)
    for op in ("and", "or", "xor", "min", "max", "sum", "prod"):
        out += c11_generic(f"shmem_{op}_reduce",
                           [f"        {ct}*: shmem_{st}_{op}_reduce" for st, ct in GENERIC_TABLE[op]])
    out += c11_generic("shmem_broadcast", [f"        {ct}*: shmem_{st}_broadcast" for st, ct in GENERIC_RMA])
    out.append("#endif")
    out += ["", "#endif /* SHMEM_REDUCTIONS_H */", ""]
    return "\n".join(out)


def source():
    out = ["// reductions_gen.cpp -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.",
           "//",
           "// The 198 typed SOS reduction entry points.  Each is SHMEM_DEF_TO_ALL or",
           "// SHMEM_DEF_REDUCE (src/collectives_c.c4:221-269): argument checks, then the",
           "// dispatcher with the (op, internal datatype) pair of bindings/shmem_bind_c.m4.",
           '#include "shmem.h"', '#include "shmemx.h"', '#include "sosx.h"',
           '#include "api_internal.h"', "",
           'extern "C" {', ""]
    for (st, ct, it), op in TO_ALL:
        name = f"shmem_{st}_{op}_to_all"
        definition(out, lambda p: to_all_sig(p, st, ct, op), name,
                   f"sos_api_to_all(target, source, nreduce, sizeof({ct}), PE_start, logPE_stride, "
                   f"PE_size, pWrk, pSync, SOSX_OP_{OPS[op]}, SOSX_DT_{it}, \"{name}\");")
    for (st, ct, it), op in REDUCE:
        name = f"shmem_{st}_{op}_reduce"
        definition(out, lambda p: reduce_sig(p, st, ct, op), name,
                   f"return sos_api_reduce(team, dest, source, nreduce, sizeof({ct}), "
                   f"SOSX_OP_{OPS[op]}, SOSX_DT_{it}, \"{name}\");")
    for st, ct in RMA:
        name = f"shmem_{st}_broadcast"
        definition(out, lambda p: bcast_sig(p, st, ct), name,
                   f"return sos_api_broadcast(team, dest, source, nelems, sizeof({ct}), PE_root, "
                   f"\"{name}\");")
    for (st, ct, it), k in SCANS:
        name = f"shmemx_{st}_sum_{k}"
        definition(out, lambda p: scan_sig(p, st, ct, k), name,
                   f"return sos_api_scan(team, dest, source, nelems, sizeof({ct}), SOSX_OP_SUM, "
                   f"SOSX_DT_{it}, {1 if k == 'exscan' else 0}, \"{name}\");")
    out += ['}  // extern "C"', ""]
    return "\n".join(out)


# fcollect / alltoall / alltoalls over the RMA table (SHMEM_BIND_C_RMA of SHMEM_DEF_FCOLLECT,
# SHMEM_DEF_ALLTOALL, SHMEM_DEF_ALLTOALLS: src/collectives_c.c4:536-558, :609-631, :687-707)
COLLECTS = ("fcollect", "alltoall", "alltoalls")
_STRIDES = {"fcollect": "", "alltoall": "", "alltoalls": "ptrdiff_t dst, ptrdiff_t sst, ", "collect": ""}
_STRIDE_ARGS = {"fcollect": "", "alltoall": "", "alltoalls": "dst, sst, ", "collect": ""}


def collect_sig(prefix, st, ct, kind):
    return (f"int {prefix}shmem_{st}_{kind}(shmem_team_t team, {ct} *dest, const {ct} *source, "
            f"{_STRIDES[kind]}size_t nelems)")


def collect_mem_sig(prefix, kind):
    return (f"int {prefix}shmem_{kind}mem(shmem_team_t team, void *dest, const void *source, "
            f"{_STRIDES[kind]}size_t nelems)")


def collect_active_sig(prefix, kind, bits):
    first = "void *target, const void *source, size_t nlong" if kind in ("fcollect", "collect") else (
        f"void *dest, const void *source, {_STRIDES[kind]}size_t nelems")
    return (f"void {prefix}shmem_{kind}{bits}({first}, int PE_start, int logPE_stride, int PE_size, "
            f"long *pSync)")


# The two generated families over the RMA table: a header and a source each.  `untyped_here`:
# the source also defines the mem and active-set forms (the collects' are written by hand).
# collect (variable lengths: SHMEM_BIND_C_RMA of SHMEM_DEF_COLLECT, shmem_collectmem and the
# deprecated shmem_collect32/64, src/collectives_c.c4:432-503) has files of its own.
FAMILIES = {
    "collects": dict(
        kinds=COLLECTS, header="shmem_collects.h", source="collects_gen.cpp", untyped_here=False,
        about_header=[" * SOS's fcollect, alltoall and alltoalls: the 72 typed team forms",
                      " * shmem_<T>_{fcollect,alltoall,alltoalls} (src/collectives_c.c4:536-707), the",
                      " * three mem forms, the six deprecated active-set forms, the C11 generic selectors",
                      " * and the C++ overloads.  Included from shmem.h. */"],
        about_source=["// The 72 typed fcollect / alltoall / alltoalls entry points (SHMEM_DEF_FCOLLECT,",
                      "// SHMEM_DEF_ALLTOALL, SHMEM_DEF_ALLTOALLS over SHMEM_BIND_C_RMA,",
                      "// src/collectives_c.c4:536-707): strong pshmem_*, weak shmem_* aliases."]),
    "collectv": dict(
        kinds=("collect",), header="shmem_collectv.h", source="collectv_gen.cpp", untyped_here=True,
        about_header=[" * SOS's collect (concatenation of per-PE contributions of different lengths): the",
                      " * 24 typed team forms shmem_<T>_collect (src/collectives_c.c4:463-485),",
                      " * shmem_collectmem, the deprecated active-set shmem_collect32/64, the C11 generic",
                      " * selector and the C++ overloads.  Included from shmem.h. */"],
        about_source=["// The 24 typed collect entry points (SHMEM_DEF_COLLECT over SHMEM_BIND_C_RMA),",
                      "// shmem_collectmem and the active-set shmem_collect32/64",
                      "// (src/collectives_c.c4:432-503): strong pshmem_*, weak shmem_* aliases."]),
}


def family_header(fam):
    guard = fam["header"].upper().replace(".", "_")
    out = [f"/* {fam['header']} -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", " *"]
    out += fam["about_header"]
    out += [f"#ifndef {guard}", f"#define {guard}", "", "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    for attr, prefix in (("SHMEM_FUNCTION_ATTRIBUTES ", ""), ("", "p")):
        if prefix:
            out.append("/* profiling interface: pshmem_* are the implementations, shmem_* weak aliases */")
        for kind in fam["kinds"]:
            for st, ct in RMA:
                out.append(f"{attr}{collect_sig(prefix, st, ct, kind)};")
            out.append(f"{attr}{collect_mem_sig(prefix, kind)};")
            for bits in (32, 64):
                out.append(f"{attr}{collect_active_sig(prefix, kind, bits)};")
            if not prefix:
                out.append("")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    out.append("#if defined(__cplusplus)")
    for kind in fam["kinds"]:
        for st, ct in GENERIC_RMA:
            out.append(f"static inline int shmem_{kind}(shmem_team_t team, {ct} *dest, const {ct} *source, "
                       f"{_STRIDES[kind]}size_t nelems) {{ return shmem_{st}_{kind}(team, dest, source, "
                       f"{_STRIDE_ARGS[kind]}nelems); }}")
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    out += c11_prelude()
    for kind in fam["kinds"]:
        out += c11_generic(f"shmem_{kind}", [f"        {ct}*: shmem_{st}_{kind}" for st, ct in GENERIC_RMA])
    out.append("#endif")
    out += ["", f"#endif /* {guard} */", ""]
    return "\n".join(out)


def family_source(fam):
    out = [f"// {fam['source']} -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", "//"]
    out += fam["about_source"]
    out += ['#include "shmem.h"', '#include "api_internal.h"', "", 'extern "C" {', ""]
    for kind in fam["kinds"]:
        for st, ct in RMA:
            name = f"shmem_{st}_{kind}"
            definition(out, lambda p: collect_sig(p, st, ct, kind), name,
                       f"return sos_api_{kind}(team, dest, source, {_STRIDE_ARGS[kind]}nelems, "
                       f"sizeof({ct}), \"{name}\");")
        if not fam["untyped_here"]:
            continue
        name = f"shmem_{kind}mem"
        definition(out, lambda p: collect_mem_sig(p, kind), name,
                   f"return sos_api_{kind}(team, dest, source, {_STRIDE_ARGS[kind]}nelems, 1, \"{name}\");")
        for bits in (32, 64):
            name = f"shmem_{kind}{bits}"
            definition(out, lambda p: collect_active_sig(p, kind, bits), name,
                       f"sos_api_{kind}_active(target, source, nlong, {bits // 8}, PE_start, logPE_stride, "
                       f"PE_size, pSync, \"{name}\");")
    out += ['}  // extern "C"', ""]
    return "\n".join(out)


# ---- one-sided put / get (SHMEM_DECLARE_FOR_RMA over the RMA table, SHMEM_DECLARE_FOR_SIZES
# over 8..128: mpp/shmem_c_func.h4:46-241, mpp/shmemx_c_func.h4:32-71, src/data_c.c4:300-680)
RMA_SIZES = (8, 16, 32, 64, 128)
_RMA_CONTIG = ("put", "get", "put_nbi", "get_nbi")
_RMA_STRIDED = ("iput", "iget")
_RMA_BLOCK = ("ibput", "ibget")
_STRIDED_ARGS = "ptrdiff_t tst, ptrdiff_t sst, size_t len, int pe"
_BLOCK_ARGS = "ptrdiff_t tst, ptrdiff_t sst, size_t bsize, size_t nblocks, int pe"


def _rma_call(kind, size, name):
    """The generic entry behind one form; `size` is a C expression for the element size."""
    if kind in _RMA_CONTIG:
        api, nbi = kind.split("_")[0], 1 if kind.endswith("_nbi") else 0
        return f'sos_api_{api}(target, source, nelems, {size}, pe, {nbi}, "{name}");'
    if kind in _RMA_STRIDED:
        return f'sos_api_{kind}(target, source, tst, sst, len, {size}, pe, "{name}");'
    return f'sos_api_{kind}(target, source, tst, sst, bsize, nblocks, {size}, pe, "{name}");'


def rma_entries():
    """(header, name, sig(prefix), body) of every generated one-sided entry; header is
    'shmem' or 'shmemx'."""
    out = []

    def add(hdr, name, proto, body):
        # proto has one "{p}" where the pshmem prefix goes
        out.append((hdr, name, lambda p, proto=proto: proto.format(p=p), body))

    for st, ct in RMA:
        for kind in _RMA_CONTIG:
            name = f"shmem_{st}_{kind}"
            add("shmem", name, f"void {{p}}{name}({ct} *target, const {ct} *source, size_t nelems, int pe)",
                _rma_call(kind, f"sizeof({ct})", name))
        name = f"shmem_{st}_p"
        add("shmem", name, f"void {{p}}{name}({ct} *addr, {ct} value, int pe)",
            f'sos_api_p(addr, &value, sizeof({ct}), pe, "{name}");')
        name = f"shmem_{st}_g"
        add("shmem", name, f"{ct} {{p}}{name}(const {ct} *addr, int pe)",
            f'{ct} tmp; sos_api_g(&tmp, addr, sizeof({ct}), pe, "{name}"); return tmp;')
        for kind in _RMA_STRIDED:
            name = f"shmem_{st}_{kind}"
            add("shmem", name, f"void {{p}}{name}({ct} *target, const {ct} *source, {_STRIDED_ARGS})",
                _rma_call(kind, f"sizeof({ct})", name))
        for kind in _RMA_BLOCK:
            name = f"shmemx_{st}_{kind}"
            add("shmemx", name, f"void {{p}}{name}({ct} *target, const {ct} *source, {_BLOCK_ARGS})",
                _rma_call(kind, f"sizeof({ct})", name))
    for bits in RMA_SIZES:
        for kind in _RMA_CONTIG:
            base, _, nbi = kind.partition("_")
            name = f"shmem_{base}{bits}" + ("_nbi" if nbi else "")
            add("shmem", name, f"void {{p}}{name}(void *target, const void *source, size_t nelems, int pe)",
                _rma_call(kind, str(bits // 8), name))
        for kind in _RMA_STRIDED:
            name = f"shmem_{kind}{bits}"
            add("shmem", name, f"void {{p}}{name}(void *target, const void *source, {_STRIDED_ARGS})",
                _rma_call(kind, str(bits // 8), name))
        for kind in _RMA_BLOCK:
            name = f"shmemx_{kind}{bits}"
            add("shmemx", name, f"void {{p}}{name}(void *target, const void *source, {_BLOCK_ARGS})",
                _rma_call(kind, str(bits // 8), name))
    for kind in _RMA_CONTIG:
        base, _, nbi = kind.partition("_")
        name = f"shmem_{base}mem" + ("_nbi" if nbi else "")
        add("shmem", name, f"void {{p}}{name}(void *target, const void *source, size_t nelems, int pe)",
            _rma_call(kind, "1", name))
    return out


def rma_symbols():
    """Every public one-sided name, shmem_ptr (written by hand in rma.cpp) included."""
    return [name for _, name, _, _ in rma_entries()] + ["shmem_ptr"]


def _rma_generic_args(kind):
    """(C++ parameter list after the two pointers, call arguments) of one generic."""
    if kind in _RMA_CONTIG:
        return "size_t nelems, int pe", "nelems, pe"
    if kind in _RMA_STRIDED:
        return _STRIDED_ARGS, "tst, sst, len, pe"
    return _BLOCK_ARGS, "tst, sst, bsize, nblocks, pe"


def _rma_generics(prefix, kinds, with_pg):
    """The C++ overloads and the C11 selectors of `kinds` (and shmem_p / shmem_g)."""
    out = ["#if defined(__cplusplus)"]
    for kind in kinds:
        params, args = _rma_generic_args(kind)
        for st, ct in GENERIC_RMA:
            out.append(f"static inline void {prefix}_{kind}({ct} *target, const {ct} *source, {params}) "
                       f"{{ {prefix}_{st}_{kind}(target, source, {args}); }}")
    if with_pg:
        for st, ct in GENERIC_RMA:
            out.append(f"static inline void shmem_p({ct} *addr, {ct} value, int pe) "
                       f"{{ shmem_{st}_p(addr, value, pe); }}")
        for st, ct in GENERIC_RMA:
            out.append(f"static inline {ct} shmem_g(const {ct} *addr, int pe) {{ return shmem_{st}_g(addr, pe); }}")
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    out += c11_prelude()
    # there is no context argument here: the selector looks at the first argument
    out += ["#ifndef SHMEM_C11_ARG0", "#define SHMEM_C11_ARG0(...) SHMEM_C11_ARG0_HELPER(__VA_ARGS__, sentinel)",
            "#define SHMEM_C11_ARG0_HELPER(first, ...) first", "#endif"]
    for kind in kinds:
        out += c11_generic(f"{prefix}_{kind}", [f"        {ct}*: {prefix}_{st}_{kind}" for st, ct in GENERIC_RMA],
                           argidx=0)
    if with_pg:
        out += c11_generic("shmem_p", [f"        {ct}*: shmem_{st}_p" for st, ct in GENERIC_RMA], argidx=0)
        out += c11_generic("shmem_g", [f"        {ct}*: shmem_{st}_g, \\\n        const {ct}*: shmem_{st}_g"
                                       for st, ct in GENERIC_RMA], argidx=0)
    out.append("#endif")
    return out


def rma_header(which):
    fname = "shmem_rma.h" if which == "shmem" else "shmemx_rma.h"
    guard = fname.upper().replace(".", "_")
    out = [f"/* {fname} -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", " *"]
    if which == "shmem":
        out += [" * SOS's one-sided put / get family on the symmetric heaps: the typed forms",
                " * shmem_<T>_{put,get,put_nbi,get_nbi,p,g,iput,iget} over the 24 RMA types, the sized",
                " * forms for 8..128 bits, putmem / getmem, shmem_ptr, the C11 generic selectors and the",
                " * C++ overloads (mpp/shmem_c_func.h4:46-241).  The shmem_ctx_* forms are in shmem_ctx.h.",
                " * Included from shmem.h. */"]
    else:
        out += [" * SOS's block-strided extension shmemx_<T>_{ibput,ibget} and shmemx_{ibput,ibget}<N>",
                " * (mpp/shmemx_c_func.h4:32-71): nblocks blocks of bsize elements, tst / sst elements",
                " * apart.  Included from shmemx.h. */"]
    out += [f"#ifndef {guard}", f"#define {guard}", "", "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    entries = [e for e in rma_entries() if e[0] == which]
    for _, name, sig, _ in entries:
        out.append(f"SHMEM_FUNCTION_ATTRIBUTES {sig('')};")
    if which == "shmem":
        out.append("SHMEM_FUNCTION_ATTRIBUTES void *shmem_ptr(const void *target, int pe);")
    out += ["", "/* profiling interface: pshmem_* are the implementations, shmem_* weak aliases */"]
    for _, name, sig, _ in entries:
        out.append(f"{sig('p')};")
    if which == "shmem":
        out.append("void *pshmem_ptr(const void *target, int pe);")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    if which == "shmem":
        out += _rma_generics("shmem", _RMA_CONTIG + _RMA_STRIDED, True)
    else:
        out += _rma_generics("shmemx", _RMA_BLOCK, False)
    out += ["", f"#endif /* {guard} */", ""]
    return "\n".join(out)


def rma_source():
    out = ["// rma_gen.cpp -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", "//",
           "// The typed, sized and mem forms of put / get / p / g / iput / iget and of SOS's",
           "// shmemx ibput / ibget (SHMEM_DEF_PUT ... SHMEM_DEF_IBGET_N over SHMEM_BIND_C_RMA and",
           "// SHMEM_BIND_C_SIZES, src/data_c.c4:300-680): strong pshmem_*, weak shmem_* aliases.",
           '#include "shmem.h"', '#include "shmemx.h"', '#include "api_internal.h"', "", 'extern "C" {', ""]
    for _, name, sig, body in rma_entries():
        definition(out, sig, name, body)
    out += ['}  // extern "C"', ""]
    return "\n".join(out)


# ---- atomic memory operations (SHMEM_DECLARE_FOR_AMO / _EXTENDED_AMO / _BITWISE_AMO:
# mpp/shmem_c_func.h4:243-404, :575-639; bindings/shmem_bind_c.m4:43-69; src/atomic_c.c4,
# src/atomic_nbi_c.c4).  The shmem_ctx_* forms: ctx_entries below.
AMO = [("int", "int"), ("long", "long"), ("longlong", "long long"), ("uint", "unsigned int"),
       ("ulong", "unsigned long"), ("ulonglong", "unsigned long long"), ("int32", "int32_t"),
       ("int64", "int64_t"), ("uint32", "uint32_t"), ("uint64", "uint64_t"), ("size", "size_t"),
       ("ptrdiff", "ptrdiff_t")]
EXTENDED_AMO = AMO + [("float", "float"), ("double", "double")]
BITWISE_AMO = [("uint", "unsigned int"), ("ulong", "unsigned long"), ("ulonglong", "unsigned long long"),
               ("int32", "int32_t"), ("int64", "int64_t"), ("uint32", "uint32_t"), ("uint64", "uint64_t")]
AMO_TABLES = {"AMO": AMO, "EXTENDED_AMO": EXTENDED_AMO, "BITWISE_AMO": BITWISE_AMO}
# the generic selectors' arms (bindings/shmem_bind_c11.m4:30-56, shmem_bind_cxx.m4:30-54)
_AMO_BASE = AMO[:6]
AMO_GENERIC_C11 = {"AMO": _AMO_BASE, "EXTENDED_AMO": _AMO_BASE + EXTENDED_AMO[-2:],
                   "BITWISE_AMO": [("int32", "int32_t"), ("int64", "int64_t")] + BITWISE_AMO[:3]}
AMO_GENERIC_CXX = {"AMO": _AMO_BASE, "EXTENDED_AMO": _AMO_BASE + EXTENDED_AMO[-2:],
                   "BITWISE_AMO": BITWISE_AMO[:3]}

# form -> (table, SOSX_AMO_* op, shape, deprecated).  shape: which operands the prototype
# has -- "v" value, "c" cond, "1" the constant one (inc) -- and whether the old value is
# returned ("r"), goes to *fetch ("n": the nbi forms) or is dropped ("").
AMO_FORMS = {}
for _form, _old, _table, _op, _args in (
        ("atomic_compare_swap", "cswap", "AMO", "CSWAP", "cv"), ("atomic_fetch_inc", "finc", "AMO", "ADD", "1"),
        ("atomic_fetch_add", "fadd", "AMO", "ADD", "v"), ("atomic_swap", "swap", "EXTENDED_AMO", "SWAP", "v"),
        ("atomic_fetch", "fetch", "EXTENDED_AMO", "FETCH", ""), ("atomic_fetch_and", None, "BITWISE_AMO", "AND", "v"),
        ("atomic_fetch_or", None, "BITWISE_AMO", "OR", "v"), ("atomic_fetch_xor", None, "BITWISE_AMO", "XOR", "v")):
    AMO_FORMS[_form] = (_table, _op, _args, "r", False)
    if _old:
        AMO_FORMS[_old] = (_table, _op, _args, "r", True)
    AMO_FORMS[_form + "_nbi"] = (_table, _op, _args, "n", False)
for _form, _old, _table, _op, _args in (
        ("atomic_inc", "inc", "AMO", "ADD", "1"), ("atomic_add", "add", "AMO", "ADD", "v"),
        ("atomic_set", "set", "EXTENDED_AMO", "SET", "v"), ("atomic_and", None, "BITWISE_AMO", "AND", "v"),
        ("atomic_or", None, "BITWISE_AMO", "OR", "v"), ("atomic_xor", None, "BITWISE_AMO", "XOR", "v")):
    AMO_FORMS[_form] = (_table, _op, _args, "", False)
    if _old:
        AMO_FORMS[_old] = (_table, _op, _args, "", True)
# what a deprecated generic selects in C++ (mpp/shmem.h4:322-387, :452-487: the new name)
_AMO_RENAMED = {"cswap": "atomic_compare_swap", "finc": "atomic_fetch_inc", "fadd": "atomic_fetch_add",
                "swap": "atomic_swap", "fetch": "atomic_fetch", "inc": "atomic_inc", "add": "atomic_add",
                "set": "atomic_set"}


def _amo_params(form, ct):
    """(parameter list, argument names) of one form for C type `ct`."""
    table, op, args, old, dep = AMO_FORMS[form]
    params = [f"{ct} *fetch"] if old == "n" else []
    params.append(f"const {ct} *target" if op == "FETCH" else f"{ct} *target")
    params += [f"{ct} cond"] if "c" in args else []
    params += [f"{ct} value"] if "v" in args else []
    params.append("int pe")
    return ", ".join(params), ", ".join(p.split()[-1].lstrip("*") for p in params)


def _amo_ret(form, ct):
    return ct if AMO_FORMS[form][3] == "r" else "void"


def amo_entries():
    """(name, sig(prefix), body, deprecated) of every generated atomic entry."""
    out = []
    for form, (table, op, args, old, dep) in AMO_FORMS.items():
        for st, ct in AMO_TABLES[table]:
            name = f"shmem_{st}_{form}"
            params, _ = _amo_params(form, ct)
            proto = f"{_amo_ret(form, ct)} {{p}}{name}({params})"
            is_float = 1 if st in ("float", "double") else 0
            pre = f"{ct} value = 1; " if "1" in args else ""
            value = "&value" if ("v" in args or "1" in args) else "NULL"
            cond = "&cond" if "c" in args else "NULL"
            target = "(void *)target" if op == "FETCH" else "target"
            fetch = {"r": "&old", "n": "fetch", "": "NULL"}[old]
            call = (f"sos_api_amo(SOSX_AMO_{op}, {target}, {value}, {cond}, {fetch}, {1 if old else 0}, "
                    f"sizeof({ct}), {is_float}, pe, {1 if old == 'n' else 0}, \"{name}\");")
            body = pre + (f"{ct} old; {call} return old;" if old == "r" else call)
            out.append((name, lambda p, proto=proto: proto.format(p=p), body, dep))
    return out


def amo_symbols():
    """Every public atomic name (typed forms; there are no untyped ones)."""
    return [name for name, _, _, _ in amo_entries()]


def _amo_generics():
    out = ["#if defined(__cplusplus)"]
    for form, (table, op, args, old, dep) in AMO_FORMS.items():
        for st, ct in AMO_GENERIC_CXX[table]:
            params, names = _amo_params(form, ct)
            ret = _amo_ret(form, ct)
            callee = f"shmem_{st}_{_AMO_RENAMED.get(form, form)}"
            out.append(f"static inline {ret} shmem_{form}({params}) "
                       f"{{ {'return ' if ret != 'void' else ''}{callee}({names}); }}")
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    out += c11_prelude()
    out += ["#ifndef SHMEM_C11_ARG0", "#define SHMEM_C11_ARG0(...) SHMEM_C11_ARG0_HELPER(__VA_ARGS__, sentinel)",
            "#define SHMEM_C11_ARG0_HELPER(first, ...) first", "#endif"]
    for form, (table, op, args, old, dep) in AMO_FORMS.items():
        arms = [f"        {ct}*: shmem_{st}_{form}" for st, ct in AMO_GENERIC_C11[table]]
        if op == "FETCH":  # the target is const: both qualifications select (mpp/shmem.h4:1013-1035)
            arms += [f"        const {ct}*: shmem_{st}_{form}" for st, ct in AMO_GENERIC_C11[table]]
        out += c11_generic(f"shmem_{form}", arms, argidx=0)
    out.append("#endif")
    return out


def amo_header():
    out = ["/* shmem_amo.h -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", " *",
           " * SOS's atomic memory operations on the symmetric heaps (mpp/shmem_c_func.h4:243-404,",
           " * :575-639): compare_swap, fetch_inc, inc, fetch_add, add over the 12 AMO types; swap,",
           " * fetch, set over those and float, double; and, or, xor and their fetching forms over the",
           " * 7 bitwise types; the deprecated pre-1.4 names; the nbi fetching forms; the C11 generic",
           " * selectors and the C++ overloads.  The shmem_ctx_* forms are in shmem_ctx.h.  Included from",
           " * shmem.h. */",
           "#ifndef SHMEM_AMO_H", "#define SHMEM_AMO_H", "",
           "#ifndef SHMEM_ATTRIBUTE_DEPRECATED",
           "#define SHMEM_ATTRIBUTE_DEPRECATED __attribute__((deprecated))", "#endif", "",
           "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    entries = amo_entries()
    for name, sig, _, dep in entries:
        out.append(f"SHMEM_FUNCTION_ATTRIBUTES {sig('')}{' SHMEM_ATTRIBUTE_DEPRECATED' if dep else ''};")
    out += ["", "/* profiling interface: pshmem_* are the implementations, shmem_* weak aliases */"]
    for name, sig, _, dep in entries:
        out.append(f"{sig('p')}{' SHMEM_ATTRIBUTE_DEPRECATED' if dep else ''};")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    out += _amo_generics()
    out += ["", "#endif /* SHMEM_AMO_H */", ""]
    return "\n".join(out)


def amo_source():
    out = ["// amo_gen.cpp -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", "//",
           "// The typed atomic memory operations (SHMEM_DEF_SWAP ... SHMEM_DEF_FETCH_XOR over",
           "// SHMEM_BIND_C_AMO, _EXTENDED_AMO and _BITWISE_AMO, src/atomic_c.c4:226-560, and the nbi",
           "// forms of src/atomic_nbi_c.c4) over amo.cpp: strong pshmem_*, weak shmem_* aliases.",
           '#include "shmem.h"', '#include "sosx.h"', '#include "api_internal.h"', "", 'extern "C" {', ""]
    for name, sig, body, _ in amo_entries():
        definition(out, sig, name, body)
    out += ['}  // extern "C"', ""]
    return "\n".join(out)


# ---- put with signal, signal operations, point-to-point synchronisation
# (mpp/shmem_c_func.h4:91-127, :473-542, :705; mpp/shmemx_c_func.h4:98-100;
# bindings/shmem_bind_c.m4:71-91; src/data_c.c4:684-784, src/synchronization_c.c4).  The
# shmem_ctx_* forms of put with signal: ctx_entries below.
WAIT = [("short", "short"), ("int", "int"), ("long", "long"), ("longlong", "long long")]
SYNC = WAIT + [("ushort", "unsigned short"), ("uint", "unsigned int"), ("ulong", "unsigned long"),
               ("ulonglong", "unsigned long long"), ("int32", "int32_t"), ("int64", "int64_t"),
               ("uint32", "uint32_t"), ("uint64", "uint64_t"), ("size", "size_t"), ("ptrdiff", "ptrdiff_t")]
_SYNC_SIGNED = {"short", "int", "long", "longlong", "int32", "int64", "ptrdiff"}
# the generic selectors' arms (bindings/shmem_bind_c11.m4:58-67, shmem_bind_cxx.m4:56-63)
SYNC_GENERIC_C11 = SYNC[:8]
SYNC_GENERIC_CXX = [t for t in SYNC[:8] if t[0] not in ("short", "ushort")]
# form -> (return type, kind, has indices, vector)
SYNC_FORMS = {}
for _w, _wret in (("wait_until", None), ("test", "int")):
    SYNC_FORMS[_w] = (_wret or "void", "ONE", False, False)
    for _vec in (False, True):
        _sfx = "_vector" if _vec else ""
        SYNC_FORMS[f"{_w}_all{_sfx}"] = (_wret or "void", "ALL", False, _vec)
        SYNC_FORMS[f"{_w}_any{_sfx}"] = ("size_t", "ANY", False, _vec)
        SYNC_FORMS[f"{_w}_some{_sfx}"] = ("size_t", "SOME", True, _vec)
_PUT_SIGNAL_ARGS = "size_t nelems, uint64_t *sig_addr, uint64_t signal, int sig_op, int pe"
_PUT_SIGNAL_NAMES = "nelems, sig_addr, signal, sig_op, pe"


def _sync_params(form, ct):
    """(parameter list, argument names) of one wait / test form for C type `ct`."""
    ret, kind, has_idx, vec = SYNC_FORMS[form]
    if kind == "ONE":
        return f"{ct} *var, int cmp, {ct} value", "var, cmp, value"
    idx = "size_t *indices, " if has_idx else ""
    val = f"{ct} *values" if vec else f"{ct} value"
    return (f"{ct} *vars, size_t nelems, {idx}const int *status, int cmp, {val}",
            f"vars, nelems, {'indices, ' if has_idx else ''}status, cmp, {'values' if vec else 'value'}")


def _sync_macro(form):
    return "SOS_" + form.upper()


def _sync_call(form, ct, signed, name):
    """The body of one wait / test form: `ct`, `signed` and `name` as C expressions."""
    ret, kind, has_idx, vec = SYNC_FORMS[form]
    ivars = "var, 1" if kind == "ONE" else "vars, nelems"
    common = (f"{ivars}, {'indices' if has_idx else 'NULL'}, {'NULL' if kind == 'ONE' else 'status'}, cmp, "
              f"{'values' if vec else '&value'}, {1 if vec else 0}, SOS_SYNC_{kind}, sizeof({ct}), {signed}")
    call = f"sos_api_wait({common}, NULL, {name});" if form.startswith("wait") else f"sos_api_test({common}, {name});"
    return call if ret == "void" else f"return {'(int)' if ret == 'int' else ''}{call}"


def signal_entries():
    """(header section, name, sig(prefix), source line, deprecated, guard) of every generated
    put-with-signal, signal and point-to-point synchronisation entry.  source line: the
    entry's one line in signal_gen.cpp, an invocation of SOS_ENTRY or of its family's macro
    (signal_macros); guard: a preprocessor condition under which the header declares it."""
    out = []

    def add(sec, name, ret, params, body=None, line=None, dep=False, guard=None):
        proto = f"{ret} {{p}}{name}({params})"
        out.append((sec, name, lambda p, proto=proto: proto.format(p=p),
                    line or f"SOS_ENTRY({ret}, {name}, ({params}), {body})", dep, guard))

    def put_signal(name, ct, size, nbi):
        add("signal", name, "void", f"{ct} *target, const {ct} *source, {_PUT_SIGNAL_ARGS}",
            line=f"SOS_PUT_SIGNAL({name}, {ct}, {size}, {nbi})")

    for nbi, sfx in ((0, ""), (1, "_nbi")):
        for st, ct in RMA:
            put_signal(f"shmem_{st}_put_signal{sfx}", ct, f"sizeof({ct})", nbi)
        for bits in RMA_SIZES:
            put_signal(f"shmem_put{bits}_signal{sfx}", "void", str(bits // 8), nbi)
        put_signal(f"shmem_putmem_signal{sfx}", "void", "1", nbi)
    add("signal", "shmem_signal_fetch", "uint64_t", "const uint64_t *sig_addr",
        'return sos_api_signal_fetch(sig_addr, "shmem_signal_fetch");')
    for op in ("add", "set"):
        name = f"shmemx_signal_{op}"
        add("signal", name, "void", "uint64_t *sig_addr, uint64_t signal, int pe",
            f'sos_api_signal_op(sig_addr, signal, SOSX_SIGNAL_{op.upper()}, pe, "{name}");')
    # the deprecated waits: until the ivar differs from value (cmp -1)
    for st, ct in WAIT:
        add("sync", f"shmem_{st}_wait", "void", f"{ct} *var, {ct} value", line=f"SOS_WAIT(shmem_{st}_wait, {ct})", dep=True)
    add("sync", "shmem_wait", "void", "long *ivar, long cmp_value",
        'sos_api_wait(ivar, 1, NULL, NULL, -1, &cmp_value, 0, SOS_SYNC_ONE, sizeof(long), 1, NULL, "shmem_wait");',
        dep=True)
    # "Special case, only enabled when C++ and C11 bindings are disabled".  signal_gen.cpp is
    # C++, where the header's overloads hold the name: the weak alias gets its symbol name
    # from an asm label
    add("sync", "shmem_wait_until", "void", "long *ivar, int cmp, long value",
        line='void pshmem_wait_until(long *ivar, int cmp, long value) { sos_api_wait(ivar, 1, NULL, NULL, cmp, &value, 0, '
             'SOS_SYNC_ONE, sizeof(long), 1, NULL, "shmem_wait_until"); }\n'
             'void sos_untyped_wait_until(long *ivar, int cmp, long value) __asm__("shmem_wait_until") '
             '__attribute__((weak, alias("pshmem_wait_until")));',
        guard="(!defined(__cplusplus) && !(defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L)) || "
              "defined(SHMEM_DECLARE_SPECIAL_CASES)")
    for form, (ret, kind, has_idx, vec) in SYNC_FORMS.items():
        for st, ct in SYNC:
            name = f"shmem_{st}_{form}"
            add("sync", name, ret, _sync_params(form, ct)[0],
                line=f"{_sync_macro(form)}({name}, {ct}, {1 if st in _SYNC_SIGNED else 0})")
    add("sync", "shmem_signal_wait_until", "uint64_t", "uint64_t *sig_addr, int cmp, uint64_t cmp_value",
        'uint64_t got = 0; sos_api_wait(sig_addr, 1, NULL, NULL, cmp, &cmp_value, 0, SOS_SYNC_ONE, sizeof(uint64_t), '
        '0, &got, "shmem_signal_wait_until"); return got;')
    return out


def signal_macros():
    """The macros signal_gen.cpp's lines invoke: SOS_ENTRY (the strong pshmem form with its
    one-line body and the weak alias) and one macro per family over (name, C type, ...)."""
    out = ["#define SOS_ENTRY(ret, name, params, ...) \\",
           "    ret p##name params { __VA_ARGS__ } \\",
           "    ret name params __attribute__((weak, alias(\"p\" #name)));",
           "#define SOS_PUT_SIGNAL(name, T, size, nbi) \\",
           f"    SOS_ENTRY(void, name, (T *target, const T *source, {_PUT_SIGNAL_ARGS}), \\",
           "              sos_api_put_signal(target, source, nelems, size, sig_addr, signal, sig_op, pe, nbi, #name);)",
           "#define SOS_WAIT(name, T) \\",
           "    SOS_ENTRY(void, name, (T *var, T value), \\",
           "              sos_api_wait(var, 1, NULL, NULL, -1, &value, 0, SOS_SYNC_ONE, sizeof(T), 1, NULL, #name);)"]
    for form, (ret, kind, has_idx, vec) in SYNC_FORMS.items():
        out += [f"#define {_sync_macro(form)}(name, T, sg) \\",
                f"    SOS_ENTRY({ret}, name, ({_sync_params(form, 'T')[0]}), \\",
                f"              {_sync_call(form, 'T', 'sg', '#name')})"]
    return out


def signal_symbols():
    """Every public put-with-signal, signal and point-to-point synchronisation name."""
    return [name for _, name, _, _, _, _ in signal_entries()]


def _signal_generics(sec):
    out = ["#if defined(__cplusplus)"]
    if sec == "signal":
        for sfx in ("", "_nbi"):
            for st, ct in GENERIC_RMA:
                out.append(f"static inline void shmem_put_signal{sfx}({ct} *dest, const {ct} *source, "
                           f"{_PUT_SIGNAL_ARGS}) {{ shmem_{st}_put_signal{sfx}(dest, source, {_PUT_SIGNAL_NAMES}); }}")
    else:
        for form, (ret, kind, has_idx, vec) in SYNC_FORMS.items():
            for st, ct in SYNC_GENERIC_CXX:
                params, names = _sync_params(form, ct)
                out.append(f"static inline {ret} shmem_{form}({params}) "
                           f"{{ {'return ' if ret != 'void' else ''}shmem_{st}_{form}({names}); }}")
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    out += c11_prelude()
    out += ["#ifndef SHMEM_C11_ARG0", "#define SHMEM_C11_ARG0(...) SHMEM_C11_ARG0_HELPER(__VA_ARGS__, sentinel)",
            "#define SHMEM_C11_ARG0_HELPER(first, ...) first", "#endif"]
    if sec == "signal":
        for sfx in ("", "_nbi"):
            out += c11_generic(f"shmem_put_signal{sfx}",
                               [f"        {ct}*: shmem_{st}_put_signal{sfx}" for st, ct in GENERIC_RMA], argidx=0)
    else:
        for form in SYNC_FORMS:
            out += c11_generic(f"shmem_{form}", [f"        {ct}*: shmem_{st}_{form}" for st, ct in SYNC_GENERIC_C11],
                               argidx=0)
    out.append("#endif")
    return out


def signal_header(sec):
    fname = "shmem_signal.h" if sec == "signal" else "shmem_sync.h"
    guard = fname.upper().replace(".", "_")
    out = [f"/* {fname} -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", " *"]
    if sec == "signal":
        out += [" * SOS's put with signal on the device symmetric heap: shmem_<T>_put_signal[_nbi] over the",
                " * 24 RMA types, the sized forms for 8..128 bits, putmem_signal[_nbi], shmem_signal_fetch",
                " * and SOS's extensions shmemx_signal_add / shmemx_signal_set (mpp/shmem_c_func.h4:91-127,",
                " * :705; mpp/shmemx_c_func.h4:98-100), with the C11 generic selectors and the C++ overloads.",
                " * The shmem_ctx_* forms are in shmem_ctx.h.  Included from shmem.h. */"]
    else:
        out += [" * SOS's point-to-point synchronisation (mpp/shmem_c_func.h4:473-542): shmem_<T>_wait_until",
                " * and shmem_<T>_test with their _all / _any / _some and _vector forms over the 14 SYNC",
                " * types, shmem_signal_wait_until, and the deprecated shmem_<T>_wait over short, int, long,",
                " * long long; the C11 generic selectors and the C++ overloads.  The untyped shmem_wait_until",
                " * is declared where SOS declares it: not under the C11 or C++ generics.  Included from",
                " * shmem.h. */"]
    out += [f"#ifndef {guard}", f"#define {guard}", ""]
    if sec == "signal":
        out += ["/* signal operations (mpp/shmem-def.h.in:116-117) */", "#define SHMEM_SIGNAL_SET 0",
                "#define SHMEM_SIGNAL_ADD 1", ""]
    else:
        out += ["/* comparisons (mpp/shmem-def.h.in:27-39) */"]
        for i, c in enumerate(("EQ", "NE", "GT", "GE", "LT", "LE")):
            out += [f"#define SHMEM_CMP_{c} {i + 1}", f"#define _SHMEM_CMP_{c} {i + 1}"]
        out += ["", "#ifndef SHMEM_ATTRIBUTE_DEPRECATED",
                "#define SHMEM_ATTRIBUTE_DEPRECATED __attribute__((deprecated))", "#endif", ""]
    out += ["#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    entries = [e for e in signal_entries() if e[0] == sec]

    def declare(attr, prefix):
        for _, name, sig, _, dep, cond in entries:
            line = f"{attr}{sig(prefix)}{' SHMEM_ATTRIBUTE_DEPRECATED' if dep else ''};"
            out.extend([f"#if {cond}", line, "#endif"] if cond else [line])

    declare("SHMEM_FUNCTION_ATTRIBUTES ", "")
    out += ["", "/* profiling interface: pshmem_* are the implementations, shmem_* weak aliases */"]
    declare("", "p")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    out += _signal_generics(sec)
    out += ["", f"#endif /* {guard} */", ""]
    return "\n".join(out)


def signal_source():
    out = ["// signal_gen.cpp -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", "//",
           "// Put with signal, the signal operations and the point-to-point waits and tests",
           "// (SHMEM_DEF_PUT_SIGNAL ... _PUT_N_SIGNAL_NBI over SHMEM_BIND_C_RMA and SHMEM_BIND_C_SIZES,",
           "// src/data_c.c4:684-784; SHMEM_DEF_WAIT ... SHMEM_DEF_TEST_SOME_VECTOR over SHMEM_BIND_C_WAIT",
           "// and SHMEM_BIND_C_SYNC, src/synchronization_c.c4) over signal.cpp: strong pshmem_*, weak",
           "// shmem_* aliases.  One line per entry point: the families stamp theirs out of a macro per",
           "// form, as SOS stamps its own out of SHMEM_DEF_* macros over its type tables.",
           '#include "shmem.h"', '#include "sosx.h"', '#include "api_internal.h"', ""]
    out += signal_macros()
    out += ["", 'extern "C" {', ""]
    out += [line for _, _, _, line, _, _ in signal_entries()]
    out += ["", '}  // extern "C"', ""]
    return "\n".join(out)


# ---- communication contexts: the ctx twin of every put, get, atomic and put-with-signal
# (mpp/shmem_c_func.h4:60-406, :547-658; mpp/shmemx_c_func.h4:32-101; the shmem_ctx_* stamping
# of src/data_c.c4:820-880).  A twin is its plain form with "ctx_" after the prefix, a leading
# shmem_ctx_t and the sos_api_ctx_* entry.  The deprecated atomics, the waits and tests,
# shmem_signal_fetch, shmem_ptr and the locks have none.
#
# The 575 twins are not written out: the headers and ctx_gen.cpp hold each FORM once, as a
# macro over (name part, C type) -- or (bits, bytes) for the sized forms -- and stamp it over
# X-macro type tables, as SOS stamps its own out of m4 tables.  ctx_entries() is the same
# expansion done here, for the name list, the Python mirrors and the tests, which compare it
# with what the preprocessor makes of the headers.
#
# The public names live in a library of their own, sos_amd/libsos_amd_ctx.so (ctx_gen.cpp
# alone), over the sos_api_ctx_* entries of libsos_amd.so: that library's export list is
# pinned to hold no shmem_ctx_ name.
CTX_MANAGEMENT = [
    ("shmem_ctx_create", "int", "long options, shmem_ctx_t *ctx", "return sos_api_ctx_create(options, ctx);"),
    ("shmem_ctx_destroy", "void", "shmem_ctx_t ctx", "sos_api_ctx_destroy(ctx);"),
    ("shmem_ctx_quiet", "void", "shmem_ctx_t ctx", "sos_api_ctx_quiet(ctx);"),
    ("shmem_ctx_fence", "void", "shmem_ctx_t ctx", "sos_api_ctx_fence(ctx);"),
    ("shmem_team_create_ctx", "int", "shmem_team_t team, long options, shmem_ctx_t *ctx",
     "return sos_api_team_create_ctx(team, options, ctx);"),
    ("shmem_ctx_get_team", "int", "shmem_ctx_t ctx, shmem_team_t *team", "return sos_api_ctx_get_team(ctx, team);")]
# X-macro tables: name -> rows (name part, second column)
CTX_TABLES = {
    "RMA": RMA, "SIZES": [(str(b), str(b // 8)) for b in RMA_SIZES],
    "SIZES_MEM": [(str(b), str(b // 8)) for b in RMA_SIZES] + [("mem", "1")],
    "AMO": AMO, "EXTENDED_AMO": EXTENDED_AMO, "BITWISE_AMO": BITWISE_AMO}
_CTX_SIZED = ("SIZES", "SIZES_MEM")   # their second column is SZ, the element's bytes; else T, its C type


def ctx_forms():
    """(header, family, table, return type, name before the type, name after it, parameters
    after ctx, body) of every ctx FORM; T / SZ stand for the table's second column, fn for the
    entry's own name."""
    out = []
    for table, ptr, size in (("RMA", "T", "sizeof(T)"), ("SIZES", "void", "SZ"), ("SIZES_MEM", "void", "SZ")):
        typed = table == "RMA"
        pre, mid = ("shmem_ctx_", "_") if typed else ("shmem_ctx_", "")
        xpre = "shmemx_ctx_"
        two = f"{ptr} *target, const {ptr} *source"
        if table != "SIZES":
            for kind in _RMA_CONTIG:
                api, _, nbi = kind.partition("_")
                out.append(("shmem", "rma", table, "void", pre + ("" if typed else api), (mid + kind) if typed else
                            ("_nbi" if nbi else ""), f"{two}, size_t nelems, int pe",
                            f"sos_api_ctx_{api}(ctx, target, source, nelems, {size}, pe, {1 if nbi else 0}, fn);"))
            for nbi, sfx in ((0, ""), (1, "_nbi")):
                out.append(("shmem", "signal", table, "void", pre + ("" if typed else "put"),
                            (mid + "put_signal" + sfx) if typed else ("_signal" + sfx), f"{two}, {_PUT_SIGNAL_ARGS}",
                            f"sos_api_ctx_put_signal(ctx, target, source, nelems, {size}, sig_addr, signal, sig_op, "
                            f"pe, {nbi}, fn);"))
        if typed:
            out.append(("shmem", "rma", table, "void", pre, "_p", "T *addr, T value, int pe",
                        "sos_api_ctx_p(ctx, addr, &value, sizeof(T), pe, fn);"))
            out.append(("shmem", "rma", table, "T", pre, "_g", "const T *addr, int pe",
                        "T tmp; sos_api_ctx_g(ctx, &tmp, addr, sizeof(T), pe, fn); return tmp;"))
        if table != "SIZES_MEM":
            for kind in _RMA_STRIDED:
                out.append(("shmem", "rma", table, "void", pre + ("" if typed else kind), (mid + kind) if typed else "",
                            f"{two}, {_STRIDED_ARGS}", f"sos_api_ctx_{kind}(ctx, target, source, tst, sst, len, {size}, pe, fn);"))
            for kind in _RMA_BLOCK:
                out.append(("shmemx", "rma", table, "void", xpre + ("" if typed else kind), (mid + kind) if typed else "",
                            f"{two}, {_BLOCK_ARGS}",
                            f"sos_api_ctx_{kind}(ctx, target, source, tst, sst, bsize, nblocks, {size}, pe, fn);"))
    for form, (table, op, args, old, dep) in AMO_FORMS.items():
        if dep:
            continue
        params, _ = _amo_params(form, "T")
        value = "&value" if ("v" in args or "1" in args) else "NULL"
        call = (f"sos_api_ctx_amo(ctx, SOSX_AMO_{op}, {'(void *)target' if op == 'FETCH' else 'target'}, {value}, "
                f"{'&cond' if 'c' in args else 'NULL'}, {{'r': '&old', 'n': 'fetch', '': 'NULL'}}, {1 if old else 0}, "
                f"sizeof(T), (T)0.5 != (T)0, pe, {1 if old == 'n' else 0}, fn);").replace(
                    "{'r': '&old', 'n': 'fetch', '': 'NULL'}", {"r": "&old", "n": "fetch", "": "NULL"}[old])
        body = ("T value = 1; " if "1" in args else "") + (f"T old; {call} return old;" if old == "r" else call)
        out.append(("shmem", "amo", table, "T" if old == "r" else "void", "shmem_ctx_", "_" + form, params, body))
    return out


def _ctx_subst(text, second, sized):
    import re
    return re.sub(r"\bSZ\b" if sized else r"\bT\b", second, text)


_CTX_SIGNAL_OPS = [(f"shmemx_ctx_signal_{op}", f"sos_api_ctx_signal_op(ctx, sig_addr, signal, SOSX_SIGNAL_{op.upper()}, pe, fn);")
                   for op in ("add", "set")]
_CTX_SIGNAL_OP_PARAMS = "uint64_t *sig_addr, uint64_t signal, int pe"


def ctx_entries():
    """(header, family, name, sig(prefix)) of every ctx twin: the forms expanded over their
    tables, and the two signal operations."""
    out = []
    for hdr, family, table, ret, pre, suf, params, _ in ctx_forms():
        sized = table in _CTX_SIZED
        for first, second in CTX_TABLES[table]:
            name = pre + first + suf
            proto = (f"{_ctx_subst(ret, second, sized)} {{p}}{name}(shmem_ctx_t ctx, "
                     f"{_ctx_subst(params, second, sized)})")
            out.append((hdr, family, name, lambda p, proto=proto: proto.format(p=p)))
    for name, _ in _CTX_SIGNAL_OPS:
        proto = f"void {{p}}{name}(shmem_ctx_t ctx, {_CTX_SIGNAL_OP_PARAMS})"
        out.append(("shmemx", "signal", name, lambda p, proto=proto: proto.format(p=p)))
    return out


def ctx_symbols():
    """Every public context name: the six management calls and the twins."""
    return [n for n, _, _, _ in CTX_MANAGEMENT] + [name for _, _, name, _ in ctx_entries()]


def _ctx_macro(head, lines):
    return [head + " \\"] + [f"    {ln} \\" for ln in lines[:-1]] + [f"    {lines[-1]}"]


def _ctx_stamp(which, macro, item):
    """One macro per table holding every form of header `which` -- item(form) is its line --
    and the table's stamping of it."""
    out = []
    for table in CTX_TABLES:
        forms = [f for f in ctx_forms() if f[0] == which and f[2] == table]
        if forms:
            second = "SZ" if table in _CTX_SIZED else "T"
            out += _ctx_macro(f"#define {macro}_{table}(N, {second})", [item(f) for f in forms])
            out += [f"SHMEM_CTX_FOR_{table}({macro}_{table})", f"#undef {macro}_{table}"]
    return out


def _ctx_name_tokens(pre, suf):
    return f"{pre}##N{'##' + suf if suf else ''}"


_CTX_C11_TABLES = {"RMA": GENERIC_RMA, "AMO": AMO_GENERIC_C11["AMO"], "EXTENDED_AMO": AMO_GENERIC_C11["EXTENDED_AMO"],
                   "BITWISE_AMO": AMO_GENERIC_C11["BITWISE_AMO"]}
_CTX_CXX_TABLES = {"RMA": GENERIC_RMA, "AMO": AMO_GENERIC_CXX["AMO"], "EXTENDED_AMO": AMO_GENERIC_CXX["EXTENDED_AMO"],
                   "BITWISE_AMO": AMO_GENERIC_CXX["BITWISE_AMO"]}


def _ctx_generic_list(which):
    """(generic name, table, ctx prefix, plain prefix, suffix, C++ return, C++ parameters, C++
    argument names, const ctx arms, const plain arms) of every generic of header `which`."""
    out = []
    if which == "shmem":
        for kind in _RMA_CONTIG + _RMA_STRIDED:
            params, args = _rma_generic_args(kind)
            out.append((f"shmem_{kind}", "RMA", "shmem_ctx_", "shmem_", f"_{kind}", "void",
                        f"T *target, const T *source, {params}", f"target, source, {args}", False, False))
        out.append(("shmem_p", "RMA", "shmem_ctx_", "shmem_", "_p", "void", "T *addr, T value, int pe", "addr, value, pe",
                    False, False))
        out.append(("shmem_g", "RMA", "shmem_ctx_", "shmem_", "_g", "T", "const T *addr, int pe", "addr, pe", True, True))
        for form, (table, op, args, old, dep) in AMO_FORMS.items():
            if not dep:
                params, names = _amo_params(form, "T")
                # the blocking fetch selects on its const target; the nbi forms on `fetch`
                out.append((f"shmem_{form}", table, "shmem_ctx_", "shmem_", f"_{form}", "T" if old == "r" else "void",
                            params, names, op == "FETCH" and old != "n", op == "FETCH"))
        for sfx in ("", "_nbi"):
            out.append((f"shmem_put_signal{sfx}", "RMA", "shmem_ctx_", "shmem_", f"_put_signal{sfx}", "void",
                        f"T *dest, const T *source, {_PUT_SIGNAL_ARGS}", f"dest, source, {_PUT_SIGNAL_NAMES}", False, False))
    else:
        for kind in _RMA_BLOCK:
            params, args = _rma_generic_args(kind)
            out.append((f"shmemx_{kind}", "RMA", "shmemx_ctx_", "shmemx_", f"_{kind}", "void",
                        f"T *target, const T *source, {params}", f"target, source, {args}", False, False))
    return out


def _ctx_generics(which):
    gens = _ctx_generic_list(which)
    out = ["#if defined(__cplusplus)"]
    if which == "shmem":
        for table, rows in _CTX_CXX_TABLES.items():
            out.append(f"#define SHMEM_CTX_FOR_CXX_{table}(X) " + " ".join(f"X({st}, {ct})" for st, ct in rows))
    for table in _CTX_CXX_TABLES:
        lines = [f"static inline {ret} {g}(shmem_ctx_t ctx, {params}) {{ {'return ' if ret != 'void' else ''}"
                 f"{cp}##N##{s}(ctx, {names}); }}" for g, t, cp, pp, s, ret, params, names, _, _ in gens if t == table]
        if lines:
            out += _ctx_macro(f"#define SHMEM_CTX_CXX_{table}(N, T)", lines)
            out += [f"SHMEM_CTX_FOR_CXX_{table}(SHMEM_CTX_CXX_{table})", f"#undef SHMEM_CTX_CXX_{table}"]
    if which == "shmemx":
        for op in ("add", "set"):
            out.append(f"static inline void shmemx_signal_{op}(shmem_ctx_t ctx, {_CTX_SIGNAL_OP_PARAMS}) "
                       f"{{ shmemx_ctx_signal_{op}(ctx, sig_addr, signal, pe); }}")
    out.append("#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L")
    if which == "shmem":
        out += c11_prelude()
        out += ["#ifndef SHMEM_C11_ARG0", "#define SHMEM_C11_ARG0(...) SHMEM_C11_ARG0_HELPER(__VA_ARGS__, sentinel)",
                "#define SHMEM_C11_ARG0_HELPER(first, ...) first", "#endif",
                "#define SHMEM_C11_TYPE_EVAL_PTR_OR_SCALAR(arg) (arg)+0",
                "/* matches no call: selecting it is a compile-time error */",
                "static inline void shmem_ctx_c11_generic_selection_failed(void) { }",
                "/* the arms of a selector over one type table: <type>*: <p><name part><s> (and the const",
                " * pointers for the forms that read their target) */"]
        for table, rows in _CTX_C11_TABLES.items():
            arms = ", ".join(f"{ct}*: p##{st}##s" for st, ct in rows)
            out.append(f"#define SHMEM_CTX_ARMS_{table}(p, s) {arms}")
            out.append(f"#define SHMEM_CTX_CARMS_{table}(p, s) SHMEM_CTX_ARMS_{table}(p, s), "
                       + ", ".join(f"const {ct}*: p##{st}##s" for st, ct in rows))
        out += ["/* a selector that takes an optional leading context: the first argument chooses between the",
                " * ctx forms (arms CA over prefix cp), selected by the second argument, and the plain forms",
                " * (arms PA over prefix pp) */"]
        out += _ctx_macro("#define SHMEM_CTX_SELECT(CA, PA, cp, pp, s, ...)",
                          ["_Generic(SHMEM_C11_TYPE_EVAL_PTR(SHMEM_C11_ARG0(__VA_ARGS__)),",
                           "    shmem_ctx_t: _Generic(SHMEM_C11_TYPE_EVAL_PTR_OR_SCALAR(SHMEM_C11_ARG1(__VA_ARGS__)),",
                           "        CA(cp, s), default: shmem_ctx_c11_generic_selection_failed),",
                           "    PA(pp, s))(__VA_ARGS__)"])
    for g, table, cp, pp, s, _, _, _, cconst, pconst in gens:
        ca = f"SHMEM_CTX_{'CARMS' if cconst else 'ARMS'}_{table}"
        pa = f"SHMEM_CTX_{'CARMS' if pconst else 'ARMS'}_{table}"
        out += [f"#undef {g}", f"#define {g}(...) SHMEM_CTX_SELECT({ca}, {pa}, {cp}, {pp}, {s}, __VA_ARGS__)"]
    if which == "shmemx":
        for op in ("add", "set"):
            out += [f"#define shmemx_signal_{op}(...) _Generic(SHMEM_C11_TYPE_EVAL_PTR(SHMEM_C11_ARG0(__VA_ARGS__)), \\",
                    f"    shmem_ctx_t: shmemx_ctx_signal_{op}, uint64_t*: shmemx_signal_{op})(__VA_ARGS__)"]
    out.append("#endif")
    return out


def ctx_header(which):
    fname = "shmem_ctx.h" if which == "shmem" else "shmemx_ctx.h"
    guard = fname.upper().replace(".", "_")
    out = [f"/* {fname} -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", " *"]
    if which == "shmem":
        out += [" * SOS's communication contexts (mpp/shmem_c_func.h4:60-406, :547-658): shmem_ctx_create /",
                " * destroy / quiet / fence, shmem_team_create_ctx, shmem_ctx_get_team, and the shmem_ctx_ twin",
                " * of every put, get, p, g, iput, iget, non-deprecated atomic and put with signal.  Each FORM",
                " * is declared once, as a macro over (name part, C type) -- (bits, bytes) for the sized forms",
                " * -- stamped over the type tables below; `cc -E` shows the prototypes written out.  The C++",
                " * overloads gain a form with a leading shmem_ctx_t, and the C11 selectors are redefined to",
                " * take one: shmem_put(ctx, dest, source, nelems, pe).  The symbols are in libsos_amd_ctx.so:",
                " * link -lsos_amd_ctx -lsos_amd.  Included last from shmem.h. */"]
    else:
        out += [" * The context twins of SOS's extensions (mpp/shmemx_c_func.h4:32-101): shmemx_ctx_<T>_{ibput,",
                " * ibget}, shmemx_ctx_ib{put,get}<N>, shmemx_ctx_signal_add / _set, with the generics taking a",
                " * leading shmem_ctx_t; declared as shmem_ctx.h declares its own.  Included last from shmemx.h. */"]
    out += [f"#ifndef {guard}", f"#define {guard}", ""]
    if which == "shmem":
        out += ["/* the type tables (bindings/shmem_bind_c.m4): X(name part, C type); sizes: X(bits, bytes) */"]
        for table, rows in CTX_TABLES.items():
            out.append(f"#define SHMEM_CTX_FOR_{table}(X) " + " ".join(f"X({a}, {b})" for a, b in rows))
        out += ["/* one entry point: the shmem_ name and its pshmem_ twin (the profiling interface) */",
                "#define SHMEM_CTX_DECL(ret, name, params) SHMEM_FUNCTION_ATTRIBUTES ret name params; ret p##name params;"]
    out += ["", "#ifdef __cplusplus", 'extern "C" {', "#endif", ""]
    if which == "shmem":
        for name, ret, params, _ in CTX_MANAGEMENT:
            out.append(f"SHMEM_CTX_DECL({ret}, {name}, ({params}))")
    else:
        for name, _ in _CTX_SIGNAL_OPS:
            out.append(f"SHMEM_CTX_DECL(void, {name}, (shmem_ctx_t ctx, {_CTX_SIGNAL_OP_PARAMS}))")
    out += _ctx_stamp(which, "SHMEM_CTX_DECL" if which == "shmem" else "SHMEMX_CTX_DECL",
                      lambda f: f"SHMEM_CTX_DECL({f[3]}, {_ctx_name_tokens(f[4], f[5])}, (shmem_ctx_t ctx, {f[6]}))")
    out += ["", "#ifdef __cplusplus", "}  /* extern \"C\" */", "#endif", ""]
    out += _ctx_generics(which)
    out += ["", f"#endif /* {guard} */", ""]
    return "\n".join(out)


def ctx_source():
    out = ["// ctx_gen.cpp -- GENERATED by sos_amd/csrc/gen_bindings.py; do not edit.", "//",
           "// libsos_amd_ctx.so: the six context management calls and the context twins of the typed, sized",
           "// and mem forms of put / get / p / g / iput / iget / ibput / ibget, of the non-deprecated atomics",
           "// and of put with signal and the signal operations (the shmem_ctx_* stamping of",
           "// src/data_c.c4:820-880 and src/atomic_c.c4) over the sos_api_ctx_* entries of libsos_amd.so:",
           "// strong pshmem_*, weak shmem_* aliases.  One macro per form, stamped over the type tables of",
           "// shmem_ctx.h; `fn` is the entry's own name.",
           '#include "shmem.h"', '#include "shmemx.h"', '#include "sosx.h"', '#include "api_internal.h"', "",
           "#define SOS_CTX_DEF(ret, name, params, ...) \\",
           "    ret p##name params { static const char fn[] = #name; (void)fn; __VA_ARGS__ } \\",
           "    ret name params __attribute__((weak, alias(\"p\" #name)));", "", 'extern "C" {', ""]
    for name, ret, params, body in CTX_MANAGEMENT:
        out.append(f"SOS_CTX_DEF({ret}, {name}, ({params}), {body})")
    for name, body in _CTX_SIGNAL_OPS:
        out.append(f"SOS_CTX_DEF(void, {name}, (shmem_ctx_t ctx, {_CTX_SIGNAL_OP_PARAMS}), {body})")
    for which in ("shmem", "shmemx"):
        out += _ctx_stamp(which, "SOS_CTX_" + which.upper(),
                          lambda f: f"SOS_CTX_DEF({f[3]}, {_ctx_name_tokens(f[4], f[5])}, (shmem_ctx_t ctx, {f[6]}), {f[7]})")
    out += ["", '}  // extern "C"', ""]
    return "\n".join(out)


def collect_symbols():
    """The generated fcollect / alltoall / alltoalls names (typed forms only)."""
    return [f"shmem_{st}_{kind}" for kind in COLLECTS for st, ct in RMA]


def collectv_symbols():
    """The generated collect names: typed, mem and active-set forms."""
    return ([f"shmem_{st}_collect" for st, ct in RMA] + ["shmem_collectmem", "shmem_collect32",
                                                         "shmem_collect64"])


def symbols():
    """All generated public names (used by the ABI test)."""
    return ([f"shmem_{st}_{op}_to_all" for (st, ct, it), op in TO_ALL]
            + [f"shmem_{st}_{op}_reduce" for (st, ct, it), op in REDUCE]
            + [f"shmem_{st}_broadcast" for st, ct in RMA]
            + [f"shmemx_{st}_sum_{k}" for (st, ct, it), k in SCANS])


def main():
    assert len(TO_ALL) == 44 and len(REDUCE) == 154, (len(TO_ALL), len(REDUCE))
    assert len(RMA) == 24 and len(SCANS) == 52, (len(RMA), len(SCANS))
    targets = {os.path.join(ROOT, "include", "shmem_reductions.h"): header(),
               os.path.join(ROOT, "include", "shmemx_scans.h"): scan_header(),
               os.path.join(ROOT, "sos_amd", "csrc", "reductions_gen.cpp"): source()}
    for fam in FAMILIES.values():
        targets[os.path.join(ROOT, "include", fam["header"])] = family_header(fam)
        targets[os.path.join(ROOT, "sos_amd", "csrc", fam["source"])] = family_source(fam)
    assert len(rma_symbols()) == 24 * 10 + 5 * 8 + 4 + 1, len(rma_symbols())
    targets[os.path.join(ROOT, "include", "shmem_rma.h")] = rma_header("shmem")
    targets[os.path.join(ROOT, "include", "shmemx_rma.h")] = rma_header("shmemx")
    targets[os.path.join(ROOT, "sos_amd", "csrc", "rma_gen.cpp")] = rma_source()
    n_amo = sum(len(AMO_TABLES[table]) for table, _, _, _, _ in AMO_FORMS.values())
    assert len(amo_symbols()) == len(set(amo_symbols())) == n_amo, (len(amo_symbols()), n_amo)
    targets[os.path.join(ROOT, "include", "shmem_amo.h")] = amo_header()
    targets[os.path.join(ROOT, "sos_amd", "csrc", "amo_gen.cpp")] = amo_source()
    n_sig = 2 * (len(RMA) + len(RMA_SIZES) + 1) + 4 + len(SYNC) * len(SYNC_FORMS) + len(WAIT) + 2
    assert len(signal_symbols()) == len(set(signal_symbols())) == n_sig == 266, (len(signal_symbols()), n_sig)
    targets[os.path.join(ROOT, "include", "shmem_signal.h")] = signal_header("signal")
    targets[os.path.join(ROOT, "include", "shmem_sync.h")] = signal_header("sync")
    targets[os.path.join(ROOT, "sos_amd", "csrc", "signal_gen.cpp")] = signal_source()
    n_ctx_amo = sum(len(AMO_TABLES[t]) for t, _, _, _, dep in AMO_FORMS.values() if not dep)
    n_ctx = len(CTX_MANAGEMENT) + (len(rma_symbols()) - 1) + n_ctx_amo + 2 * (len(RMA) + len(RMA_SIZES) + 1) + 2
    assert len(ctx_symbols()) == len(set(ctx_symbols())) == n_ctx, (len(ctx_symbols()), n_ctx)
    targets[os.path.join(ROOT, "include", "shmem_ctx.h")] = ctx_header("shmem")
    targets[os.path.join(ROOT, "include", "shmemx_ctx.h")] = ctx_header("shmemx")
    targets[os.path.join(ROOT, "sos_amd", "csrc", "ctx_gen.cpp")] = ctx_source()
    check = "--check" in sys.argv
    stale = False
    for path, text in targets.items():
        old = open(path).read() if os.path.exists(path) else None
        if old != text:
            stale = True
            if not check:
                with open(path, "w") as fh:
                    fh.write(text)
    if check and stale:
        print("generated bindings are stale", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
