// pc_consensus.hip -- one round of the UMI consensus on the device: the pile-up of every member on its group's template and
// the call of the votes (the rule: pc_consensus.h).
//
// consensus_pileup_kernel<CPL, STRANDED>: ONE WAVE PER (member, template) PAIR, a block is one wave.  The wave sweeps the band row by
// row; lane t owns the CPL = ceil(W / 64) consecutive cells k = t CPL .. t CPL + CPL - 1 of every row (W = 2 band + 1).
//   * The previous row lives in LDS (W dwords).  A row's band starts sh = centre(i) - centre(i - 1) columns to the right of
//     the row above, so cell k reads the old cells k + sh (above) and k + sh - 1 (diagonal): two LDS reads at a wave-uniform
//     shift, whatever the shift.  centre(i) = floor(i lb / la) is carried by quotient and remainder: no division in the loop.
//   * The dependence on the cell to the left is a min-plus prefix: D[k] = k + min over k' <= k of (t[k'] - k') with t = the
//     minimum of the diagonal and the vertical step.  Each lane scans its own cells, the wave scans the lanes' last cells
//     in six steps, and the values are those of the serial recurrence, so the trace is too.
//   * No global load stands in the row loop: 256 bases of the template and a window of 1 024 bases of the member are staged
//     in LDS and refilled by the whole wave when a row leaves them (a global load in the loop made every row wait for the
//     row before's trace store as well: loads and stores share one counter).
//   * The wave's scan runs in the vector ALU (DPP row shifts and broadcasts), not through the LDS crossbar.
//   * Each lane packs the two-bit choices of its cells into ONE BYTE and the wave stores the row as one line of 64 bytes:
//     the trace of a pair is (la + 1) * 64 bytes, slice member p's at trace + p * rows * 64.
//   * Only fences of wavefront scope stand between the LDS writes of a row and the reads of the next: a block is one wave.
//   * After the last row the wave decides (pcc::rejected), and for an accepted member walks the path back (pcc::walk, the
//     code the host test runs).  All 64 lanes walk the one path together, so that they can refill the walk's view together:
//     64 trace rows (4 KB, sixteen bytes a lane and load) and 256 member bases are staged in LDS, and a step reads LDS, not
//     HBM.  Lane 0 adds the votes with integer atomics: the sums do not depend on the order of arrival.
//   * STRAND.  With ConsensusArgs.member_strand the instantiations <CPL, true> run and read a member whose strand is 1 as its
//     reverse complement: the two places that fetch a member's bytes from global memory -- the s_member refill of the row loop
//     and StagedSeq's refill for the walk -- go through pcc::member_byte, wave-uniform on the member's strand (a block is one
//     wave and one member).  Everything after the staging is the same code; the votes land in template coordinates either
//     way.  Without member_strand <CPL, false> runs: the kernel as it was, instruction for instruction.
//   * A template or member length outside its range, a member of a group outside the slice or a walk that leaves its band
//     adds one to the context's error word; such a member is ST_INVALID and casts no vote.
//
// consensus_call_kernel: one block of 256 per group.  A thread takes position p: gap p's slots, then column p (adding the
// template's own vote to the column first); the bytes it emits (at most five, packed in a register) are placed by a block-wide
// prefix sum, chunk after chunk of 256 positions.  It leaves voters[g] = accepted members + tmpl_counts.
//
// consensus_call_kernel<true>: the same call (one body; <false> is consensus_call_kernel as it was, instruction for
// instruction) that also leaves ONE QUALITY BYTE PER EMITTED BASE.  When a thread emits a base the counters that decided it are in its registers:
// it turns them into the base's vote margin (pcc::column_margin, pcc::slot_margin), looks the margin up in the caller's table
// of 256 Phred values -- staged in LDS once per block, the index differs from lane to lane --, packs the up to five quality
// bytes beside its base bytes and stores them at the same offsets of a second array.  The table and the quality pointer come in
// an argument struct of the kernel's own (ConsensusQualityArgs): ConsensusArgs keeps its layout.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "pc_consensus.h"
#include "pc_kernels.h"

namespace pck {

namespace {

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The minimum over the lanes BELOW this one (INT32_MAX for lane 0): the wave's prefix scan in the vector ALU -- four shifts
// inside the rows of 16 lanes, two row broadcasts, one shift of the whole wave; no LDS crossbar.
__device__ __forceinline__ int32_t wave_min_before(int32_t x)
{
    constexpr int32_t kNone = 0x7fffffff;
    x = min(x, __builtin_amdgcn_update_dpp(kNone, x, 0x111, 0xf, 0xf, false));       // row_shr:1
    x = min(x, __builtin_amdgcn_update_dpp(kNone, x, 0x112, 0xf, 0xf, false));       // row_shr:2
    x = min(x, __builtin_amdgcn_update_dpp(kNone, x, 0x114, 0xf, 0xf, false));       // row_shr:4
    x = min(x, __builtin_amdgcn_update_dpp(kNone, x, 0x118, 0xf, 0xf, false));       // row_shr:8
    x = min(x, __builtin_amdgcn_update_dpp(kNone, x, 0x142, 0xa, 0xf, false));       // row_bcast:15 into rows 1 and 3
    x = min(x, __builtin_amdgcn_update_dpp(kNone, x, 0x143, 0xc, 0xf, false));       // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_update_dpp(kNone, x, 0x138, 0xf, 0xf, false);            // wave_shr:1
}

constexpr int kTmplRows = 256;                             // template bases staged at once for the fill
constexpr int kMemberWin = 1024;                           // member bases staged at once for the fill (a row needs at most 255)

struct VoteAdder {
    uint32_t *v;
    bool mine;                                             // every lane walks the path; one of them votes
    __device__ void operator()(int64_t counter) const { if (mine) atomicAdd(v + counter, 1u); }
};

constexpr int kWalkRows = 64;                              // trace rows staged at once: one 16-byte chunk x 4 per lane
constexpr int kWalkBases = 256;                            // member bases staged at once

// The walk's view of a pair's trace: the rows [first, first + kWalkRows) ending at the row last asked for, in LDS.  All 64
// lanes walk together (the path is one, so every branch is wave-uniform) and refill together; the walk only moves to lower rows.
struct StagedTrace {
    const uint8_t *g;                                      // the pair's trace, 64-byte aligned
    uint8_t *lds;                                          // kWalkRows * 64 bytes, 16-byte aligned
    int64_t first;
    int la, lane;
    __device__ uint8_t operator()(int64_t i, int byte)
    {
        if (i < first || i >= first + kWalkRows) {
            wave_sync();                                   // the reads of the rows staged before are done
            first = i >= kWalkRows ? i - (kWalkRows - 1) : 0;
#pragma unroll
            for (int t = 0; t < kWalkRows * pcc::TRACE_ROW_BYTES / 16 / 64; ++t) {
                const int chunk = t * 64 + lane;           // 16 bytes; four chunks a row
                if (first + chunk / 4 <= (int64_t)la)      // the pair's trace ends with row la
                    ((uint4 *)lds)[chunk] = ((const uint4 *)(g + first * pcc::TRACE_ROW_BYTES))[chunk];
            }
            wave_sync();
        }
        return lds[(i - first) * pcc::TRACE_ROW_BYTES + byte];
    }
};

// The member's bases [first, first + kWalkBases) in LDS, refilled so that the base asked for is the window's last.  STRANDED:
// a member with `reverse` set is staged as its reverse complement (pcc::member_byte).
template <bool STRANDED>
struct StagedSeq {
    const uint8_t *g;
    uint8_t *lds;
    int64_t first;
    int lb, lane;
    bool reverse;
    static constexpr int kUnroll = STRANDED ? 1 : kWalkBases / 64;     // (see consensus_pileup_kernel)
    __device__ uint8_t operator()(int64_t j)
    {
        if (j < first || j >= first + kWalkBases) {
            wave_sync();
            first = j >= kWalkBases ? j - (kWalkBases - 1) : 0;
#pragma unroll kUnroll
            for (int t = 0; t < kWalkBases / 64; ++t) {
                const int64_t at = first + t * 64 + lane;
                if (at < (int64_t)lb) lds[t * 64 + lane] = STRANDED ? pcc::member_byte(g, lb, at, reverse) : g[at];
            }
            wave_sync();
        }
        return lds[j - first];
    }
};

// STRANDED: the member's strand is read once, at the top, and kept as ONE scalar (a byte load lands in a vector register, and a
// comparison of that would hold a lane mask), and the three refills stay ROLLED loops: the row loop stands at the ceiling of
// the scalar registers, and with the refills unrolled as they are without the strand the flag spilled two to four of them;
// rolled, the kernel needs one scalar register fewer than without the strand.
template <int CPL, bool STRANDED>
__global__ __launch_bounds__(64) void consensus_pileup_kernel(ConsensusArgs a)
{
    __shared__ int32_t s_row[64 * CPL];
    __shared__ uint4 s_trace[kWalkRows * pcc::TRACE_ROW_BYTES / 16];
    __shared__ uint8_t s_bases[kWalkBases];
    __shared__ uint8_t s_tmpl[kTmplRows];
    __shared__ uint8_t s_member[kMemberWin];

    const int lane = threadIdx.x;
    const int64_t slot = blockIdx.x, m = a.first_member + slot;
    const bool reverse = STRANDED && __builtin_amdgcn_readfirstlane((int)a.member_strand[m]) != 0;
    constexpr int kUnrollMember = STRANDED ? 1 : kMemberWin / 64, kUnrollTmpl = STRANDED ? 1 : kTmplRows / 64;       // (full without the strand)
    int32_t *out = a.member_out + 2 * m;
    const int64_t g = a.member_group[m];
    int la = 0, lb = a.member_len[m];
    bool fine = g >= a.first_group && g < a.first_group + a.n_groups;
    if (fine) {
        la = a.tmpl_len[g];
        fine = la >= 1 && la <= a.max_len && (int64_t)la < a.rows && lb >= 0 && lb <= a.max_len;
    }
    if (!fine) {
        if (lane == 0) { atomicAdd(a.err, 1u); out[0] = pcc::ST_INVALID; out[1] = -1; }
        return;
    }
    const uint8_t *ta = a.tmpl_arena + a.tmpl_off[g], *mb = a.arena + a.member_off[m];
    uint8_t *trace = a.trace + slot * a.rows * pcc::TRACE_ROW_BYTES;
    const int band = a.band, W = 2 * band + 1;

    // row 0: D[0][j] = j
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int k = lane * CPL + c, j = k - band;
        s_row[k] = (k < W && j >= 0 && j <= lb) ? j : pcc::INF;
    }
    wave_sync();

    const int q = lb / la, r = lb % la;
    int64_t centre = 0, lo = -band;
    int acc = 0;
    int t_first = -kTmplRows;                              // s_tmpl holds the template's bases [t_first, t_first + kTmplRows): nothing yet
    int64_t m_first = 0, m_end = 0;                        // s_member holds the member's bases [m_first, m_end): nothing yet
    for (int i = 1; i <= la; ++i) {
        centre += q;
        acc += r;
        if (acc >= la) { acc -= la; ++centre; }
        const int64_t lo_new = centre - band, sh64 = lo_new - lo;
        const int sh = sh64 > (int64_t)W ? W + 1 : (int)sh64;
        if (i - 1 >= t_first + kTmplRows) {                // (wave-uniform) the next kTmplRows bases of the template
            wave_sync();
            t_first = i - 1;
#pragma unroll kUnrollTmpl
            for (int t = 0; t < kTmplRows / 64; ++t) {
                const int at = t_first + t * 64 + lane;
                if (at < la) s_tmpl[t * 64 + lane] = ta[at];
            }
            wave_sync();
        }
        const int ca = pcc::code(s_tmpl[i - 1 - t_first]);
        // the row's cells read the member's bases [need_lo, need_hi): at most W of them, and both ends only ever rise
        const int64_t need_lo = lo_new > 1 ? lo_new - 1 : 0, need_hi = lo_new + W - 1 < (int64_t)lb ? lo_new + W - 1 : (int64_t)lb;
        if (need_hi > need_lo && (need_lo < m_first || need_hi > m_end)) {
            wave_sync();
            m_first = need_lo;
            m_end = m_first + kMemberWin < (int64_t)lb ? m_first + kMemberWin : (int64_t)lb;
#pragma unroll kUnrollMember
            for (int t = 0; t < kMemberWin / 64; ++t) {
                const int64_t at = m_first + t * 64 + lane;
                if (at < m_end) s_member[t * 64 + lane] = STRANDED ? pcc::member_byte(mb, lb, at, reverse) : mb[at];
            }
            wave_sync();
        }
        uint8_t base[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int64_t j = lo_new + lane * CPL + c;
            base[c] = (j >= 1 && j <= (int64_t)lb && lane * CPL + c < W) ? s_member[j - 1 - m_first] : (uint8_t)0;
        }
        int32_t up[CPL], dg0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int at = lane * CPL + c + sh;
            up[c] = at < W ? s_row[at] : pcc::INF;
        }
        {
            const int at = lane * CPL + sh - 1;
            dg0 = (at >= 0 && at < W) ? s_row[at] : pcc::INF;
        }
        wave_sync();                                      // every lane has read the old row

        int32_t dv[CPL], uv[CPL], x[CPL];
        bool valid[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int k = lane * CPL + c;
            const int64_t j = lo_new + k;
            valid[c] = k < W && j >= 0 && j <= (int64_t)lb;
            const int32_t dg = c == 0 ? dg0 : up[c > 0 ? c - 1 : 0];
            const int cb = pcc::code(base[c]);
            dv[c] = (valid[c] && j >= 1) ? dg + ((ca == cb && ca < 4) ? 0 : 1) : pcc::INF;
            uv[c] = up[c] + 1;
            const int32_t t = valid[c] ? min(dv[c], uv[c]) : pcc::INF;
            x[c] = t - k;
            if (c > 0) x[c] = min(x[c], x[c - 1]);
        }
        const int32_t excl = wave_min_before(x[CPL - 1]);
        uint32_t byte = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int k = lane * CPL + c;
            int32_t v = min(x[c], excl) + k;
            int op = pcc::OP_INS;
            if (!valid[c] || v > pcc::INF) v = pcc::INF;
            if (valid[c]) op = (dv[c] == v) ? pcc::OP_DIAG : (uv[c] == v ? pcc::OP_DEL : pcc::OP_INS);
            byte |= (uint32_t)op << (2 * c);
            s_row[k] = v;
        }
        trace[(int64_t)i * pcc::TRACE_ROW_BYTES + lane] = (uint8_t)byte;
        wave_sync();
        lo = lo_new;
    }
    __syncthreads();                                      // the trace stores of all lanes, before the walk reads them
    const int32_t d = s_row[band];
    int status = pcc::ST_ACCEPTED;
    if (pcc::rejected(d, la, lb, a.max_err_pct)) {
        status = pcc::ST_REJECTED;
    } else {
        VoteAdder votes{a.votes + (a.vote_off[g] - a.vote_base), lane == 0};
        StagedTrace staged{trace, (uint8_t *)s_trace, (int64_t)la + 1, la, lane};          // (first = la + 1: nothing staged yet)
        StagedSeq<STRANDED> bases{mb, s_bases, (int64_t)lb + 1, lb, lane, reverse};
        if (!pcc::walk(bases, la, lb, band, staged, votes)) status = pcc::ST_INVALID;
    }
    if (lane != 0) return;
    out[0] = status;
    out[1] = d;
    if (status == pcc::ST_ACCEPTED) atomicAdd(a.voters + g, 1);
    if (status == pcc::ST_INVALID) atomicAdd(a.err, 1u);
}

// QUAL: the argument struct is ConsensusQualityArgs, whose table is staged in LDS first; without it the kernel is the call as it
// was, instruction for instruction.
template <bool QUAL>
__global__ __launch_bounds__(256) void consensus_call_kernel(typename std::conditional<QUAL, ConsensusQualityArgs, ConsensusArgs>::type args)
{
    __shared__ int32_t s_scan[256];

    const int tid = threadIdx.x;
    const ConsensusArgs *args_a;
    const uint8_t *s_qtab = nullptr;
    uint8_t *qual_all = nullptr;
    if constexpr (QUAL) {
        __shared__ uint8_t s_table[pcc::QUAL_ENTRIES];
        static_assert(pcc::QUAL_ENTRIES == 256, "one table entry per thread of the block");
        s_table[tid] = args.qtab[tid];
        __syncthreads();
        s_qtab = s_table;
        qual_all = args.qual;
        args_a = &args.a;
    } else {
        args_a = &args;
    }
    const ConsensusArgs &a = *args_a;
    const int64_t g = a.first_group + blockIdx.x;
    const int la = a.tmpl_len[g];
    if (la < 1 || la > a.max_len) {
        if (tid == 0) { atomicAdd(a.err, 1u); a.cons_len[g] = 0; }
        return;
    }
    uint32_t *v = a.votes + (a.vote_off[g] - a.vote_base);
    const uint8_t *ta = a.tmpl_arena + a.tmpl_off[g];
    uint8_t *cons = a.cons + a.cons_off[g];
    uint8_t *qual = QUAL ? qual_all + a.cons_off[g] : nullptr;
    const uint32_t voters = (uint32_t)(a.voters[g] + a.tmpl_counts);
    int64_t base = 0;
    for (int64_t p0 = 0; p0 <= la; p0 += 256) {
        const int64_t p = p0 + tid;
        uint64_t bytes = 0, quals = 0;
        int n = 0;
        if (p <= la) {
#pragma unroll
            for (int s = 0; s < pcc::INS_SLOTS; ++s) {
                const int c = pcc::call_slot(v + pcc::slot_counter(la, p, s, 0), voters);
                if (c >= 0) {
                    bytes |= (uint64_t)pcc::letter(c) << (8 * n);
                    if (QUAL) quals |= (uint64_t)s_qtab[pcc::quality_index(pcc::slot_margin(v + pcc::slot_counter(la, p, s, 0), voters, c))] << (8 * n);
                    ++n;
                }
            }
            if (p < la) {
                const int tc = pcc::code(ta[p]);
                if (tc < 4) v[pcc::col_counter(p, tc)] += 1u;          // the template's own vote: this thread is the column's only writer now
                const int c = pcc::call_column(v + pcc::col_counter(p, 0), tc);
                if (c < 4) {
                    bytes |= (uint64_t)pcc::letter(c) << (8 * n);
                    if (QUAL) quals |= (uint64_t)s_qtab[pcc::quality_index(pcc::column_margin(v + pcc::col_counter(p, 0), tc, a.tmpl_counts, c))] << (8 * n);
                    ++n;
                }
            }
        }
        s_scan[tid] = n;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const int t = tid >= s ? s_scan[tid - s] : 0;
            __syncthreads();
            s_scan[tid] += t;
            __syncthreads();
        }
        const int64_t at = base + s_scan[tid] - n;
        for (int t = 0; t < n; ++t) cons[at + t] = (uint8_t)(bytes >> (8 * t));
        if (QUAL)
            for (int t = 0; t < n; ++t) qual[at + t] = (uint8_t)(quals >> (8 * t));
        base += s_scan[255];
        __syncthreads();
    }
    if (tid == 0) {
        a.cons_len[g] = (int32_t)base;
        a.voters[g] = (int32_t)voters;
    }
}

}  // namespace

int launch_consensus_pileup(const ConsensusArgs &a, void *stream)
{
    if (a.n_members <= 0) return 0;
    const dim3 grid((unsigned)a.n_members), block(64);
    const int cpl = pcc::cells_per_lane(a.band);
    if (cpl < 1 || cpl > 4) return 1;
#define PCK_PILEUP(STRANDED)                                                                                                    \
    switch (cpl) {                                                                                                              \
    case 1: hipLaunchKernelGGL((consensus_pileup_kernel<1, STRANDED>), grid, block, 0, (hipStream_t)stream, a); break;          \
    case 2: hipLaunchKernelGGL((consensus_pileup_kernel<2, STRANDED>), grid, block, 0, (hipStream_t)stream, a); break;          \
    case 3: hipLaunchKernelGGL((consensus_pileup_kernel<3, STRANDED>), grid, block, 0, (hipStream_t)stream, a); break;          \
    default: hipLaunchKernelGGL((consensus_pileup_kernel<4, STRANDED>), grid, block, 0, (hipStream_t)stream, a); break;         \
    }
    if (!a.member_strand) {
        PCK_PILEUP(false)                                  // instruction for instruction the kernels from before the strands
    } else {
        PCK_PILEUP(true)
    }
#undef PCK_PILEUP
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_consensus_call(const ConsensusArgs &a, void *stream)
{
    if (a.n_groups <= 0) return 0;
    hipLaunchKernelGGL(consensus_call_kernel<false>, dim3((unsigned)a.n_groups), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_consensus_call_quality(const ConsensusQualityArgs &q, void *stream)
{
    if (q.a.n_groups <= 0) return 0;
    if (!q.qual) return 1;
    hipLaunchKernelGGL(consensus_call_kernel<true>, dim3((unsigned)q.a.n_groups), dim3(256), 0, (hipStream_t)stream, q);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace pck
