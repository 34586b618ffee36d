// pc_paths.hip -- alignment PATHS, one LANE per alignment, 64 to a one-wave block, any scoring scheme pcs::fits accepts,
// adapters of the context's table of letter sets (up to 128 bases; pc_letters.h), each lane its own.  Three kernels over one routine:
//   path_kernel         a (window, adapter) pair against the whole window: pcpath::align_path (pc_paths.h), the very
//                       function tests/host/test_paths.cpp replays base by base against the oracle;
//   middle_path_kernel  a middle hit: pcpath::align_path_window over a window of a few hundred columns of the hit's
//                       trimmed read (pc_middle_paths.h: the columns pc_bounds.h proves the hit's path and its warm-up
//                       can touch), with the read masked as the hit's round of mask-and-realign saw it: the intervals
//                       of the read's earlier hits read as code 4.  tests/host/test_middle_paths.cpp compares that very function with
//                       align_path over the whole masked read.
//   umi_kernel          an end window against ONE adapter with a span of degenerate rows: align_path_sets as in
//                       path_kernel, then pcu::extract (pc_umi.h) over the lane's own operations -- the read columns under
//                       the span.  No operation leaves the device.
// Nothing of the packed kernels is touched: paths are wanted for the few alignments somebody looks at, not for a scan.
//
// Layout: the column state (M, H per adapter row) sits in LDS as [row][lane] -- consecutive lanes in consecutive banks,
// conflict-free -- sized from the longest adapter of the table (at most 64 KB per wave).  The trace, eight rows to a
// dword, sits in a library-owned scratch as [local column][row group][alignment of the launch]: a wave's store of one
// row group is 256 contiguous bytes; the traceback's loads are per-lane gathers.  Lanes run to their own window length
// and their own adapter length.  Every index into arena, scratch, interval table and outputs is formed in 64 bits; read
// bytes are fetched as bytes and only from inside the lane's window.  A middle lane loops over its mask_count intervals
// per column: hits per read are few, and these kernels are latency-bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pc_kernels.h"
#include "pc_middle_paths.h"
#include "pc_paths.h"
#include "pc_record.h"
#include "pc_umi.h"

namespace pck {

namespace {

struct PathMem {
    int *st; int rows, lane;              // rows: the launch's LDS rows (longest adapter of the table)
    uint32_t *tr; int64_t G, P, p;        // G: row groups per column of the scratch, P: alignments of the launch, p: this lane's
    __device__ __forceinline__ int &M(int i) { return st[(i - 1) * 64 + lane]; }
    __device__ __forceinline__ int &H(int i) { return st[(rows + i - 1) * 64 + lane]; }
    __device__ __forceinline__ void put(int j, int g, uint32_t w) { tr[((int64_t)(j - 1) * G + g) * P + p] = w; }
    __device__ __forceinline__ uint32_t get(int j, int g) const { return tr[((int64_t)(j - 1) * G + g) * P + p]; }
};

// record, head and error count of alignment q of the call.  The outputs are taken as pointers: a reference to the kernel's
// argument struct costs middle_path_kernel four SGPRs and 18 instructions of prologue.
__device__ __forceinline__ void store_path(int32_t *records, int32_t *heads, uint32_t *errs, int64_t q, const pcw::Digest &d,
                                           const int32_t head[4], int err)
{
    if (err) atomicAdd(errs, 1u);
    int32_t *o = records + q * TRACE_OUT_INTS;
    ((int4 *)o)[0] = make_int4(d.read_start, d.read_end, d.adapter_start, d.adapter_end);
    ((int4 *)o)[1] = make_int4(d.score, d.matches, d.aligned_len, d.full_len);
    ((int4 *)(heads + q * 4))[0] = make_int4(head[0], head[1], head[2], head[3]);
}

__global__ __launch_bounds__(64) void path_kernel(PathArgs a)
{
    extern __shared__ int dyn[];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;       // pair of the launch
    if (p >= a.count) return;
    const int64_t q = a.first + p;                           // pair of the call
    const int n = a.seq_len[q];
    const int ai = a.adapter_idx[q];
    // the host sized the trace from max_len and the LDS from the table: a pair outside either writes nothing
    if (n < 0 || n > a.max_len || ai < 0 || ai >= a.nadapters) {
        atomicAdd(a.err, 1u);
        return;
    }
    const int m = a.ad_len[ai];
    if (m > a.rows) {
        atomicAdd(a.err, 1u);
        return;
    }
    const uint8_t *rd = a.arena + a.seq_off[q];
    const uint32_t *ad = a.ad_sets + (int64_t)ai * kMaxRows;       // the rows' sets of read codes (pc_letters.h), one per dword
    uint32_t *ops = a.ops + q * a.ops_pitch;
    const int64_t pitch = a.ops_pitch;
    pcw::Digest d;
    int32_t head[4];
    const int err = pcpath::align_path_sets(
        n, m, [&](int k) { return pcc::dna5_code(rd[k]); }, [&](int k) { return ad[k]; }, a.match, a.mismatch, a.gap_open,
        a.gap_extend, PathMem{dyn, a.rows, lane, a.trace, (int64_t)a.groups, a.P, p}, d, head,
        [&](int k, uint32_t w) { if (k < pitch) ops[k] = w; });
    store_path(a.records, a.heads, a.err, q, d, head, err);
}

__global__ __launch_bounds__(64) void middle_path_kernel(MiddlePathArgs a)
{
    extern __shared__ int dyn[];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;       // hit of the launch
    if (p >= a.count) return;
    const int64_t q = a.first + p;                           // hit of the call
    const int n = a.seq_len[q];
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
    const uint8_t *rd = a.arena + a.seq_off[q];
    const uint32_t *ad = a.ad_sets + (int64_t)ai * kMaxRows;       // the rows' sets of read codes (pc_letters.h), one per dword
    const int2 *iv = (const int2 *)a.intervals + mb;
    uint32_t *ops = a.ops + q * a.ops_pitch;
    const int64_t pitch = a.ops_pitch;
    pcw::Digest d;
    int32_t head[4];
    const int err = pcpath::align_path_window_sets(
        n, m, c0, c1,
        [&](int k) {
            int code = pcc::dna5_code(rd[k]);
            for (int t = 0; t < mc; ++t) {
                const int2 v = iv[t];
                if (k >= v.x && k < v.y) code = 4;
            }
            return code;
        },
        [&](int k) { return ad[k]; }, a.match, a.mismatch, a.gap_open, a.gap_extend,
        PathMem{dyn, a.rows, lane, a.trace, (int64_t)a.groups, a.P, p}, d, head,
        [&](int k, uint32_t w) { if (k < pitch) ops[k] = w; });
    store_path(a.records, a.heads, a.err, q, d, head, err);
}

// The UMI of one end window per lane (pc_umi.h): path_kernel's alignment against ONE adapter, uniform over the launch --
// its rows, its span and the rule are scalars, and the LDS holds this adapter's rows, not the table's longest.  The
// operations go to the launch's scratch as [word][lane of the launch] (a wave's store of one word is 256 contiguous
// bytes); the lane that wrote them reads them back, last word first, and keeps only {status, first, len, covered}.
__global__ __launch_bounds__(64) void umi_kernel(UmiArgs a)
{
    extern __shared__ int dyn[];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;       // window of the launch
    if (p >= a.count) return;
    const int64_t q = a.first + p;                           // window of the call
    const int n = a.win_len[q];
    // the host sized the trace and the operations from max_len: a window outside writes nothing
    if (n < 0 || n > a.max_len) {
        atomicAdd(a.err, 1u);
        return;
    }
    const uint8_t *rd = a.arena + a.win_off[q];
    const uint32_t *ad = a.ad_sets;
    uint32_t *ops = a.ops + p;
    const int64_t P = a.P, words = a.ops_words;
    pcw::Digest d;
    int32_t head[4];
    const int err = pcpath::align_path_sets(
        n, a.m, [&](int k) { return pcc::dna5_code(rd[k]); }, [&](int k) { return ad[k]; }, a.match, a.mismatch, a.gap_open,
        a.gap_extend, PathMem{dyn, a.m, lane, a.trace, (int64_t)a.groups, P, p}, d, head,
        [&](int k, uint32_t w) { if (k < words) ops[(int64_t)k * P] = w; });
    // a walk that left its operations: nothing of it is read back, nothing is written
    if (err || head[0] < 0 || (int64_t)head[0] > words * pcpath::OPS_PER_WORD) {
        atomicAdd(a.err, 1u);
        return;
    }
    const Rec rec = {d.read_start, d.read_end, d.adapter_start, d.adapter_end, d.score, d.matches, d.aligned_len, d.full_len};
    struct { int32_t end_size, min_trim_size; double end_threshold; } rule = {a.end_size, a.min_trim_size, a.end_threshold};
    int4 u = make_int4(0, -1, 0, 0);
    if (rec.rs < 0) u.x = 1;
    else if (a.ruled && !pcu::qualifies(rec, a.side, rule, [](int matches, int len) { return identity(matches, len); })) u.x = 2;
    else {
        const pcu::Umi e = pcu::extract(head, [&](int k) { return ops[(int64_t)k * P]; }, a.u0, a.u1);
        u = make_int4(e.complete ? 0 : 3, e.first, e.len, e.covered);
    }
    int32_t *o = a.records + q * TRACE_OUT_INTS;
    ((int4 *)o)[0] = make_int4(rec.rs, rec.re, rec.as, rec.ae);
    ((int4 *)o)[1] = make_int4(rec.score, rec.matches, rec.aligned_len, rec.full_len);
    ((int4 *)(a.umi + q * 4))[0] = u;
}

template <typename Args>
int launch(void (*kernel)(Args), const Args &a, void *stream)
{
    if (a.count <= 0) return 0;
    const unsigned grid = (unsigned)((a.count + 63) / 64);
    const size_t lds = (size_t)a.rows * 2 * 64 * sizeof(int);
    (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

int launch_paths(const PathArgs &a, void *stream) { return launch(path_kernel, a, stream); }
int launch_middle_paths(const MiddlePathArgs &a, void *stream) { return launch(middle_path_kernel, a, stream); }

int launch_umi(const UmiArgs &a, void *stream)
{
    if (a.count <= 0) return 0;
    const unsigned grid = (unsigned)((a.count + 63) / 64);
    const size_t lds = (size_t)a.m * 2 * 64 * sizeof(int);          // the CALL's adapter: at most 128 rows, 64 KB
    (void)hipFuncSetAttribute((const void *)umi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipLaunchKernelGGL(umi_kernel, dim3(grid), dim3(64), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace pck
