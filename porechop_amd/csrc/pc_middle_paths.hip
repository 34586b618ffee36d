// pc_middle_paths.hip -- the PATHS of middle hits: one LANE per hit, 64 hits per one-wave block.  The arithmetic is
// pcpath::align_path_window (pc_middle_paths.h), the very function tests/host/test_middle_paths.cpp compares with
// pcpath::align_path over the whole masked read.  A lane aligns its adapter against a window of a few hundred columns
// of its trimmed read -- the columns pc_bounds.h proves the hit's path and its warm-up can touch -- and sees the read
// masked as the hit's round of mask-and-realign saw it: the intervals of the read's earlier hits read as code 4.
//
// Layout: path_kernel's (pc_paths.hip).  The column state (M, H per adapter row) sits in LDS as [row][lane], sized from
// the longest adapter of the table; the trace, eight rows to a dword, in a library-owned scratch as
// [local column][row group][hit of the launch].  Every index into arena, scratch, interval table and outputs is formed
// in 64 bits; read bytes are fetched as bytes and only from inside the window [read_off + c0, read_off + c1).  A lane
// loops over its mask_count intervals per column: hits per read are few, and this kernel is latency-bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pc_kernels.h"
#include "pc_middle_paths.h"

namespace pck {

namespace {

__device__ __forceinline__ int mpath_code_of(uint8_t c)
{
    // seqan/basic/alphabet_residue_tabs.h:113-140
    if (c == 'A' || c == 'a') return 0;
    if (c == 'C' || c == 'c') return 1;
    if (c == 'G' || c == 'g') return 2;
    if (c == 'T' || c == 't' || c == 'U' || c == 'u') return 3;
    return 4;
}

struct MiddlePathMem {
    int *st; int rows, lane;              // rows: the launch's LDS rows (longest adapter of the table)
    uint32_t *tr; int64_t G, P, p;        // G: row groups per column of the scratch, P: hits of the launch, p: this lane's
    __device__ __forceinline__ int &M(int i) { return st[(i - 1) * 64 + lane]; }
    __device__ __forceinline__ int &H(int i) { return st[(rows + i - 1) * 64 + lane]; }
    __device__ __forceinline__ void put(int j, int g, uint32_t w) { tr[((int64_t)(j - 1) * G + g) * P + p] = w; }
    __device__ __forceinline__ uint32_t get(int j, int g) const { return tr[((int64_t)(j - 1) * G + g) * P + p]; }
};

__global__ __launch_bounds__(64) void middle_path_kernel(MiddlePathArgs a)
{
    extern __shared__ int dyn[];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;       // hit of the launch
    if (p >= a.count) return;
    const int64_t q = a.first + p;                           // hit of the call
    const int n = a.read_len[q];
    const int ai = a.adapter_idx[q];
    const int re = a.read_end[q];
    const int64_t mb = a.mask_base[q];
    const int mc = a.mask_count[q];
    // the host sized the trace from max_len and the table's bounds, the LDS from the table, and the interval table has
    // one row per hit of the call: a hit outside any of them writes nothing
    if (n < 0 || n > a.max_len || ai < 0 || ai >= a.nadapters || re < 0 || re > n || mc < 0 || mb < 0 || mb > a.n ||
        (int64_t)mc > a.n - mb) {
        atomicAdd(a.err, 1u);
        return;
    }
    const int m = a.ad_len[ai];
    const int window = a.ad_window[ai];                      // 0: compute_bounds refuses the scheme for this adapter
    const int W = window - a.ad_span[ai] - 1;
    int c0, c1;
    pcpath::hit_window(n, re, window > 0, W, window, c0, c1);
    if (m > a.rows || c1 - c0 > a.max_cols) {
        atomicAdd(a.err, 1u);
        return;
    }
    const uint8_t *rd = a.arena + a.read_off[q];
    const uint32_t *ad = a.ad_codes + (int64_t)ai * kMaxRows;      // Dna5 codes, one per dword
    const int2 *iv = (const int2 *)a.intervals + mb;
    uint32_t *ops = a.ops + q * a.ops_pitch;
    const int64_t pitch = a.ops_pitch;
    pcw::Digest d;
    int32_t head[4];
    const int err = pcpath::align_path_window(
        n, m, c0, c1,
        [&](int k) {
            int code = mpath_code_of(rd[k]);
            for (int t = 0; t < mc; ++t) {
                const int2 v = iv[t];
                if (k >= v.x && k < v.y) code = 4;
            }
            return code;
        },
        [&](int k) { return (int)ad[k]; }, a.match, a.mismatch, a.gap_open, a.gap_extend,
        MiddlePathMem{dyn, a.rows, lane, a.trace, (int64_t)a.groups, a.P, p}, d, head,
        [&](int k, uint32_t w) { if (k < pitch) ops[k] = w; });
    if (err) atomicAdd(a.err, 1u);
    int32_t *o = a.records + q * TRACE_OUT_INTS;
    ((int4 *)o)[0] = make_int4(d.read_start, d.read_end, d.adapter_start, d.adapter_end);
    ((int4 *)o)[1] = make_int4(d.score, d.matches, d.aligned_len, d.full_len);
    ((int4 *)(a.heads + q * 4))[0] = make_int4(head[0], head[1], head[2], head[3]);
}

}  // namespace

int launch_middle_paths(const MiddlePathArgs &a, void *stream)
{
    if (a.count <= 0) return 0;
    const unsigned grid = (unsigned)((a.count + 63) / 64);
    const size_t lds = (size_t)a.rows * 2 * 64 * sizeof(int);
    (void)hipFuncSetAttribute((const void *)middle_path_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipLaunchKernelGGL(middle_path_kernel, dim3(grid), dim3(64), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace pck
