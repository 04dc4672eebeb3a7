// tvr_host.h — host-only helpers of the translation units that define C-ABI entry points (tvr_api.hip, tvr_train_api.hip, tvr_mesh_api.hip): the short name of tvr_set_error, HIP_TRY
// (tvr_kernels.h), alignment, and the byte check of an fp32 matrix.  Everything here is a macro or has internal linkage: libtvr.so exports nothing from this file.
#pragma once
#include "tvr_kernels.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#define fail tvr_set_error

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// an output (or gradient input) matrix of `rows` x `cols` fp32 must have been allocated with at least that many bytes: checked on the host,
// before anything is launched (round 2's device fault was a caller buffer 144 - sum(app_n_comp) columns short of the kernel's row width)
static int need_bytes(const char *fn, const char *what, size_t have, int64_t rows, int cols)
{
    const size_t want = (size_t)rows * (size_t)cols * sizeof(float);
    if (have < want)
        return fail(TVR_ERR_SCRATCH, "%s: %s holds %zu B, the kernel writes %lld rows x %d fp32 = %zu B", fn, what, have, (long long)rows, cols, want);
    return TVR_OK;
}
// a check that returns a status, inside a function that returns one: the first refusal is the call's
#define TRY(check)                                                       \
    do {                                                                 \
        int rc_ = (check);                                               \
        if (rc_ != TVR_OK) return rc_;                                   \
    } while (0)
// NEED_FN: where the checks of two entry points share one body, which is handed the name the message carries
#define NEED_FN(fn, what, have, rows, cols) TRY(need_bytes((fn), what, (have), (rows), (cols)))
#define NEED(what, have, rows, cols) NEED_FN(__func__, what, have, rows, cols)
