// pc_record.h -- one alignment record as the per-read kernels of phase B read it (pc_reduce.hip, pc_explain.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pc_kernels.h"

namespace pck {

struct Rec { int32_t rs, re, as, ae, score, matches, aligned_len, full_len; };

// one 32-byte record as two 16-byte loads: adjacent threads read adjacent records (coalesced per job)
__device__ __forceinline__ Rec load_rec(const int32_t *base, int64_t idx)
{
    const int4 a = ((const int4 *)(base + idx * TRACE_OUT_INTS))[0];
    const int4 b = ((const int4 *)(base + idx * TRACE_OUT_INTS))[1];
    return {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// Identities are the doubles Python sees: (100.0 * matches) / length printed with %f and parsed back, i.e. rounded
// half-to-even at 6 decimals (porechop/src/alignment.cpp:113-121, nanopore_read.py:476-491)
__device__ __forceinline__ double identity(int matches, int len)
{
    const double x = (100.0 * (double)matches) / (double)len;      // 0/0 -> NaN: compares false, like Python's nan
    return rint(x * 1e6) / 1e6;
}

// a failed alignment (field 0 == -1) scores 0.0, and so does a score-only record (field 0 == -2) left untraced
__device__ __forceinline__ double full_identity(const Rec &r)
{
    return r.rs < 0 ? 0.0 : identity(r.matches, r.full_len);
}

}  // namespace pck
