// ctx_checks.cpp -- the checks of the communication contexts as plain functions of data,
// so that every refusal can be exercised without a running job (tests/test_ctx_checks.py,
// tests/ctx_checks_harness.cpp).  No HIP include; ctx.cpp builds their input from the
// runtime state and raises what they refuse.
//
//  * sos_ctx_check: a handle is LOOKED UP in the table of live contexts and never
//    dereferenced -- SHMEM_CTX_INVALID, a handle that was destroyed and any other pointer
//    are refused with a message; then the call's `pe`, an index of the context's team
//    (SOS: shmem_internal_team_pe before the checks, src/data_c.c4:829-835), becomes the
//    world PE start + pe * stride.  An index outside the team gets put / get's own bad-PE
//    message;
//  * sos_ctx_options_check: SHMEM_CTX_PRIVATE | _SERIALIZED | _NOSTORE and nothing else;
//  * sos_ctx_pool_size / sos_ctx_stream_slot: how many streams created contexts share
//    (SHMEMX_CTX_STREAMS, 1..31, default 3) and which one the n-th context gets.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>

#include "api_internal.h"

#define REFUSE(code, ...)                            \
    do {                                             \
        if (msg && n) snprintf(msg, n, __VA_ARGS__); \
        return code;                                 \
    } while (0)

extern "C" int sos_ctx_check(const sos_ctx_table *t, const void *handle, int *pe, int *index, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    if (index) *index = -1;
    if (!handle) REFUSE(SOS_CTX_INVALID, "Argument \"ctx\" is SHMEM_CTX_INVALID");
    const sos_ctx_entry *e = nullptr;
    for (int i = 0; i < t->nlive && !e; ++i)
        if (t->live[i].handle == handle) {
            e = &t->live[i];
            if (index) *index = i;
        }
    if (!e) {
        for (int i = 0; i < t->ndead; ++i)
            if (t->dead[i] == handle)
                REFUSE(SOS_CTX_DESTROYED, "Argument \"ctx\" (%p) is a context that was destroyed", handle);
        REFUSE(SOS_CTX_UNKNOWN, "Argument \"ctx\" (%p) is not a context of this library", handle);
    }
    if (!pe) return SOS_CTX_OK;
    if (*pe < 0 || *pe >= e->size) REFUSE(SOS_CTX_BAD_PE, "PE argument (%d) is invalid", *pe);
    *pe = e->start + *pe * e->stride;
    return SOS_CTX_OK;
}

extern "C" int sos_ctx_options_check(long options, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    const long known = SHMEM_CTX_PRIVATE | SHMEM_CTX_SERIALIZED | SHMEM_CTX_NOSTORE;
    if (options & ~known)
        REFUSE(SOS_CTX_BAD_OPTIONS, "Argument \"options\" (0x%lx) has bits outside SHMEM_CTX_PRIVATE | "
               "SHMEM_CTX_SERIALIZED | SHMEM_CTX_NOSTORE", (unsigned long)options);
    return SOS_CTX_OK;
}

extern "C" int sos_ctx_pool_size(const char *v, char *msg, size_t n)
{
    if (msg && n) msg[0] = 0;
    if (!v || !*v) return 3;
    char *end = nullptr;
    errno = 0;
    const long k = strtol(v, &end, 10);
    if (errno || *end || k < 1 || k > 31) REFUSE(-1, "SHMEMX_CTX_STREAMS=%s is not a number in 1..31", v);
    return (int)k;
}

extern "C" int sos_ctx_stream_slot(unsigned long created, int pool_size)
{
    return pool_size > 0 ? (int)(created % (unsigned long)pool_size) : 0;
}
