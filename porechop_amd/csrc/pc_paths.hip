// pc_paths.hip -- alignment PATHS: one LANE per (window, adapter) pair, any scoring scheme pcs::fits accepts, adapters of
// the context's code table (up to 128 bases), each lane its own.  The arithmetic is pcpath::align_path (pc_paths.h), the
// very function tests/host/test_paths.cpp replays base by base against the oracle.  Nothing of the packed kernels, of
// pc_walk.h or of pc_slow.* is touched: paths are wanted for the few pairs somebody looks at, not for a scan.
//
// Layout: the column state (M, H per adapter row) sits in LDS as [row][lane] -- consecutive lanes in consecutive banks,
// conflict-free -- sized from the longest adapter of the table (at most 64 KB per wave).  The trace, eight rows to a
// dword, sits in a library-owned scratch as [column][row group][pair of the launch]: a wave's store of one row group is
// 256 contiguous bytes; the traceback's loads are per-lane gathers.  Lanes run to their own window length and their own
// adapter length.  Every index into arena, scratch and outputs is formed in 64 bits; window bytes are read as bytes and
// nothing outside [win_off, win_off + win_len) is touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pc_kernels.h"
#include "pc_paths.h"

namespace pck {

namespace {

__device__ __forceinline__ int path_code_of(uint8_t c)
{
    // seqan/basic/alphabet_residue_tabs.h:113-140
    if (c == 'A' || c == 'a') return 0;
    if (c == 'C' || c == 'c') return 1;
    if (c == 'G' || c == 'g') return 2;
    if (c == 'T' || c == 't' || c == 'U' || c == 'u') return 3;
    return 4;
}

struct PathMem {
    int *st; int rows, lane;              // rows: the launch's LDS rows (longest adapter of the table)
    uint32_t *tr; int64_t G, P, p;        // G: row groups per column of the scratch, P: pairs of the launch, p: this lane's
    __device__ __forceinline__ int &M(int i) { return st[(i - 1) * 64 + lane]; }
    __device__ __forceinline__ int &H(int i) { return st[(rows + i - 1) * 64 + lane]; }
    __device__ __forceinline__ void put(int j, int g, uint32_t w) { tr[((int64_t)(j - 1) * G + g) * P + p] = w; }
    __device__ __forceinline__ uint32_t get(int j, int g) const { return tr[((int64_t)(j - 1) * G + g) * P + p]; }
};

__global__ __launch_bounds__(64) void path_kernel(PathArgs a)
{
    extern __shared__ int dyn[];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;       // pair of the launch
    if (p >= a.count) return;
    const int64_t q = a.first + p;                           // pair of the call
    const int n = a.win_len[q];
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
    const uint8_t *rd = a.arena + a.win_off[q];
    const uint32_t *ad = a.ad_codes + (int64_t)ai * kMaxRows;      // Dna5 codes, one per dword
    uint32_t *ops = a.ops + q * a.ops_pitch;
    const int64_t pitch = a.ops_pitch;
    pcw::Digest d;
    int32_t head[4];
    const int err = pcpath::align_path(
        n, m, [&](int k) { return path_code_of(rd[k]); }, [&](int k) { return (int)ad[k]; }, a.match, a.mismatch, a.gap_open,
        a.gap_extend, PathMem{dyn, a.rows, lane, a.trace, (int64_t)a.groups, a.P, p}, d, head,
        [&](int k, uint32_t w) { if (k < pitch) ops[k] = w; });
    if (err) atomicAdd(a.err, 1u);
    int32_t *o = a.records + q * TRACE_OUT_INTS;
    ((int4 *)o)[0] = make_int4(d.read_start, d.read_end, d.adapter_start, d.adapter_end);
    ((int4 *)o)[1] = make_int4(d.score, d.matches, d.aligned_len, d.full_len);
    ((int4 *)(a.heads + q * 4))[0] = make_int4(head[0], head[1], head[2], head[3]);
}

}  // namespace

int launch_paths(const PathArgs &a, void *stream)
{
    if (a.count <= 0) return 0;
    const unsigned grid = (unsigned)((a.count + 63) / 64);
    const size_t lds = (size_t)a.rows * 2 * 64 * sizeof(int);
    (void)hipFuncSetAttribute((const void *)path_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipLaunchKernelGGL(path_kernel, dim3(grid), dim3(64), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace pck
