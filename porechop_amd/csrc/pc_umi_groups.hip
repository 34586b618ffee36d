// pc_umi_groups.hip -- which UMI keys lie within max_dist edits of one another: the all-against-all pass behind UMI groups.
//
// umi_neighbours_kernel<Word>: every pair i < j of n keys (pc_umi_dist.h: two bit planes and a length 0 .. 64) whose
// Levenshtein distance is <= max_dist is appended to a capped list as {i, j, distance}; the cursor counts every such pair
// whether or not it fitted.  Word is uint32_t when no key is above 32 bases, uint64_t otherwise.
//
// Shape.  The keys are cut into tiles of 256; a block of 256 threads takes one pair of tiles (I, J), I <= J -- the upper
// triangle, numbered k = J (J + 1) / 2 + I, blocks striding over k so that any n fits one launch.
//   * Each lane keeps ITS key of tile I in registers: the four match masks, the length, the composition in one word.
//   * Tile J is staged in LDS (256 x {p0, p1, length, composition}: 4 or 6 KB) and every lane walks the same j.  All lanes
//     of a wave read one LDS address -- a broadcast, no bank conflict -- and the values are made scalars (readfirstlane): the
//     base of each column picks the lane's match mask by a scalar condition, and the column loop has one trip count.
//   * A lane whose lower bound (pcud::lower_bound_packed: one sum of absolute byte differences) exceeds max_dist sits the pair
//     out; a wave in which every lane sits out skips the DP of that j by a ballot.  In a diagonal block (I == J) the lanes
//     with i >= j sit out the same way, so a wave skips the j below its first lane.  The ballot fires when the 64 keys of a
//     wave resemble each other: callers order the keys by length and composition (umi_groups.kernel_order).
//   * A block whose two tiles' length ranges lie more than max_dist apart goes on to its next tile pair at once (callers
//     that order their keys by length get whole tiles skipped).
//   * Hits are rare: a wave appends with one ballot, one popcount and ONE returning atomic add on the cursor by its first
//     hit lane; the lanes store their triples with plain dword stores when their slot is below cap.
//   * A key whose length is outside 0 .. max_len has no pairs and adds one to the context's error word, once: in the
//     diagonal block that holds it.
// prune == 0 (PC_UMI_NO_PRUNE=1) runs the DP for every pair of valid keys: no bound, no tile skip.
//
// umi_neighbours_stranded_kernel<Word> (further down) is the same pass over both strands: a kernel of its own, so that the one
// above stays instruction for instruction what it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pc_kernels.h"
#include "pc_umi_dist.h"

namespace pck {

namespace {

constexpr int kTile = 256;
constexpr int kWaves = kTile / 64;

template <typename Word> __device__ __forceinline__ Word uniform(Word v);
template <> __device__ __forceinline__ uint32_t uniform<uint32_t>(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
template <> __device__ __forceinline__ uint64_t uniform<uint64_t>(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s));
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s));
    return v;
}

__device__ __forceinline__ int lower_bound_device(uint32_t ca, int la, uint32_t cb, int lb)
{
    // v_sad_u8: the four |n_a[c] - n_b[c]| summed in one instruction; (SAD + |la - lb|) / 2 as pcud::lower_bound_packed
    return (int)(__builtin_amdgcn_sad_u8(ca, cb, (uint32_t)abs(la - lb)) >> 1);
}

template <typename Word>
__global__ __launch_bounds__(kTile) void umi_neighbours_kernel(UmiNeighboursArgs a)
{
    __shared__ Word s_p0[kTile], s_p1[kTile];
    __shared__ int32_t s_len[kTile];
    __shared__ uint32_t s_comp[kTile];
    __shared__ int32_t s_range[kWaves][4];               // per wave: min, max of the lanes' keys (tile I), of the staged keys (tile J)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    const int64_t total = tiles * (tiles + 1) / 2;

    for (int64_t k = blockIdx.x; k < total; k += gridDim.x) {
        // k = J (J + 1) / 2 + I, I <= J
        int64_t J = (int64_t)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
        while (J > 0 && J * (J + 1) / 2 > k) --J;
        while ((J + 1) * (J + 2) / 2 <= k) ++J;
        const int64_t I = k - J * (J + 1) / 2;

        // the lane's own key
        const int64_t i = I * kTile + tid;
        int la = -1;
        pcud::Key own = {0, 0};
        if (i < a.n) {
            la = a.len[i];
            own.p0 = a.planes[2 * i];
            own.p1 = a.planes[2 * i + 1];
            if (la < 0 || la > a.max_len) {
                if (I == J) atomicAdd(a.err, 1u);
                la = -1;
            }
        }
        const bool valid = la >= 0;
        const Word eq0 = pcud::match_mask<Word>(own, la, 0), eq1 = pcud::match_mask<Word>(own, la, 1),
                   eq2 = pcud::match_mask<Word>(own, la, 2), eq3 = pcud::match_mask<Word>(own, la, 3);
        const uint32_t comp = valid ? pcud::composition(own, la) : 0u;
        const int top = la > 0 ? la - 1 : 0;

        // tile J into LDS
        const int64_t js = J * kTile + tid;
        int ls = -1;
        pcud::Key staged = {0, 0};
        if (js < a.n) {
            ls = a.len[js];
            staged.p0 = a.planes[2 * js];
            staged.p1 = a.planes[2 * js + 1];
            if (ls < 0 || ls > a.max_len) ls = -1;
        }
        __syncthreads();                                 // the previous tile pair's readers are done
        s_p0[tid] = (Word)staged.p0;
        s_p1[tid] = (Word)staged.p1;
        s_len[tid] = ls;
        s_comp[tid] = ls >= 0 ? pcud::composition(staged, ls) : 0u;
        {
            const int lo_i = wave_min(valid ? la : INT32_MAX), hi_i = wave_max(la);
            const int lo_j = wave_min(ls >= 0 ? ls : INT32_MAX), hi_j = wave_max(ls);
            if (lane == 0) { s_range[wave][0] = lo_i; s_range[wave][1] = hi_i; s_range[wave][2] = lo_j; s_range[wave][3] = hi_j; }
        }
        __syncthreads();
        int lo_i = INT32_MAX, hi_i = -1, lo_j = INT32_MAX, hi_j = -1;
        for (int w = 0; w < kWaves; ++w) {
            lo_i = min(lo_i, s_range[w][0]); hi_i = max(hi_i, s_range[w][1]);
            lo_j = min(lo_j, s_range[w][2]); hi_j = max(hi_j, s_range[w][3]);
        }
        if (hi_i < 0 || hi_j < 0) continue;              // a tile without a valid key
        if (a.prune && (lo_j - hi_i > a.max_dist || lo_i - hi_j > a.max_dist)) continue;

        const int jn = (int)min((int64_t)kTile, a.n - J * kTile);
        const int jfirst = (I == J) ? 1 : 0;             // j = 0 of a diagonal block has no i below it
        for (int jj = jfirst; jj < jn; ++jj) {
            const int lb = __builtin_amdgcn_readfirstlane(s_len[jj]);
            if (lb < 0) continue;
            bool act = valid && (I < J || tid < jj);
            if (a.prune) {
                const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_comp[jj]);
                act = act && lower_bound_device(comp, la, cb, lb) <= a.max_dist;
            }
            if (__ballot(act) == 0ull) continue;
            const Word t0 = uniform<Word>(s_p0[jj]), t1 = uniform<Word>(s_p1[jj]);
            Word Pv = (Word)pcud::len_mask(la), Mv = 0;
            int score = la;
            for (int t = 0; t < lb; ++t) {
                const bool b0 = (t0 >> t) & 1u, b1 = (t1 >> t) & 1u;
                const Word eq = b1 ? (b0 ? eq3 : eq2) : (b0 ? eq1 : eq0);
                pcud::column<Word>(eq, top, Pv, Mv, score);
            }
            if (la == 0) score = lb;
            const bool hit = act && score <= a.max_dist;
            const unsigned long long hits = __ballot(hit);
            if (hits != 0ull) {
                const int leader = __ffsll(hits) - 1;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(a.found, (unsigned long long)__popcll(hits));
                base = __shfl(base, leader);
                if (hit) {
                    const int64_t slot = (int64_t)(base + (unsigned long long)__popcll(hits & ((1ull << lane) - 1ull)));
                    if (slot < a.cap) {
                        int32_t *o = a.pairs + slot * 3;
                        o[0] = (int32_t)i;
                        o[1] = (int32_t)(J * kTile + jj);
                        o[2] = score;
                    }
                }
            }
        }
    }
}

// The DP of every lane's key (its match masks eq0 .. eq3, la bases) against ONE text key of lb bases given as scalar planes.
template <typename Word>
__device__ __forceinline__ int distance_to_text(Word t0, Word t1, int lb, int la, int top, Word eq0, Word eq1, Word eq2, Word eq3)
{
    Word Pv = (Word)pcud::len_mask(la), Mv = 0;
    int score = la;
    for (int t = 0; t < lb; ++t) {
        const bool b0 = (t0 >> t) & 1u, b1 = (t1 >> t) & 1u;
        const Word eq = b1 ? (b0 ? eq3 : eq2) : (b0 ? eq1 : eq0);
        pcud::column<Word>(eq, top, Pv, Mv, score);
    }
    return la == 0 ? lb : score;
}

// umi_neighbours_stranded_kernel<Word>: umi_neighbours_kernel's shape with a second comparison -- every pair i < j is compared
// as the keys stand (d_same) and with key j mirrored (d_mirror = d(key i, pcud::mirror(key j)): the other strand of the molecule),
// and is appended as {i, j, min of the two, flip} when that minimum is <= max_dist; flip = 1 iff d_mirror < d_same.
//   * While tile J is staged every thread also stages the mirror of its staged key: two more Word arrays in LDS, computed once
//     per tile pair.  The mirrored composition needs none: it is the byte reversal of s_comp[jj].
//   * Lengths do not change under mirroring: the tile-level skip and s_range are the unstranded kernel's.
//   * Per j there are two bounds and two ballots; a wave with no lane left for a comparison skips that DP.  Both DPs run over the
//     lane's own eq0 .. eq3, only the scalar text planes differ.  A lane that sat a comparison out takes no distance from it: the
//     bound put that comparison above max_dist, so the minimum over the comparisons it ran is exact whenever it is <= max_dist,
//     and so is flip (a comparison that was skipped cannot be the smaller one of a reported pair, nor tie with it).
//   * prune == 0 runs both DPs for every valid pair.
template <typename Word>
__global__ __launch_bounds__(kTile) void umi_neighbours_stranded_kernel(UmiNeighboursArgs a)
{
    __shared__ Word s_p0[kTile], s_p1[kTile], s_m0[kTile], s_m1[kTile];
    __shared__ int32_t s_len[kTile];
    __shared__ uint32_t s_comp[kTile];
    __shared__ int32_t s_range[kWaves][4];               // per wave: min, max of the lanes' keys (tile I), of the staged keys (tile J)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    const int64_t total = tiles * (tiles + 1) / 2;

    for (int64_t k = blockIdx.x; k < total; k += gridDim.x) {
        // k = J (J + 1) / 2 + I, I <= J
        int64_t J = (int64_t)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
        while (J > 0 && J * (J + 1) / 2 > k) --J;
        while ((J + 1) * (J + 2) / 2 <= k) ++J;
        const int64_t I = k - J * (J + 1) / 2;

        // the lane's own key
        const int64_t i = I * kTile + tid;
        int la = -1;
        pcud::Key own = {0, 0};
        if (i < a.n) {
            la = a.len[i];
            own.p0 = a.planes[2 * i];
            own.p1 = a.planes[2 * i + 1];
            if (la < 0 || la > a.max_len) {
                if (I == J) atomicAdd(a.err, 1u);
                la = -1;
            }
        }
        const bool valid = la >= 0;
        const Word eq0 = pcud::match_mask<Word>(own, la, 0), eq1 = pcud::match_mask<Word>(own, la, 1),
                   eq2 = pcud::match_mask<Word>(own, la, 2), eq3 = pcud::match_mask<Word>(own, la, 3);
        const uint32_t comp = valid ? pcud::composition(own, la) : 0u;
        const int top = la > 0 ? la - 1 : 0;

        // tile J into LDS, as it stands and mirrored
        const int64_t js = J * kTile + tid;
        int ls = -1;
        pcud::Key staged = {0, 0};
        if (js < a.n) {
            ls = a.len[js];
            staged.p0 = a.planes[2 * js];
            staged.p1 = a.planes[2 * js + 1];
            if (ls < 0 || ls > a.max_len) ls = -1;
        }
        const pcud::Key mirrored = pcud::mirror(staged, ls);          // (the empty key for ls <= 0)
        __syncthreads();                                 // the previous tile pair's readers are done
        s_p0[tid] = (Word)staged.p0;
        s_p1[tid] = (Word)staged.p1;
        s_m0[tid] = (Word)mirrored.p0;
        s_m1[tid] = (Word)mirrored.p1;
        s_len[tid] = ls;
        s_comp[tid] = ls >= 0 ? pcud::composition(staged, ls) : 0u;
        {
            const int lo_i = wave_min(valid ? la : INT32_MAX), hi_i = wave_max(la);
            const int lo_j = wave_min(ls >= 0 ? ls : INT32_MAX), hi_j = wave_max(ls);
            if (lane == 0) { s_range[wave][0] = lo_i; s_range[wave][1] = hi_i; s_range[wave][2] = lo_j; s_range[wave][3] = hi_j; }
        }
        __syncthreads();
        int lo_i = INT32_MAX, hi_i = -1, lo_j = INT32_MAX, hi_j = -1;
        for (int w = 0; w < kWaves; ++w) {
            lo_i = min(lo_i, s_range[w][0]); hi_i = max(hi_i, s_range[w][1]);
            lo_j = min(lo_j, s_range[w][2]); hi_j = max(hi_j, s_range[w][3]);
        }
        if (hi_i < 0 || hi_j < 0) continue;              // a tile without a valid key
        if (a.prune && (lo_j - hi_i > a.max_dist || lo_i - hi_j > a.max_dist)) continue;

        const int jn = (int)min((int64_t)kTile, a.n - J * kTile);
        const int jfirst = (I == J) ? 1 : 0;             // j = 0 of a diagonal block has no i below it
        for (int jj = jfirst; jj < jn; ++jj) {
            const int lb = __builtin_amdgcn_readfirstlane(s_len[jj]);
            if (lb < 0) continue;
            const bool pair = valid && (I < J || tid < jj);
            bool act_same = pair, act_mirror = pair;
            if (a.prune) {
                const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_comp[jj]);
                act_same = pair && lower_bound_device(comp, la, cb, lb) <= a.max_dist;
                act_mirror = pair && lower_bound_device(comp, la, pcud::mirror_composition(cb), lb) <= a.max_dist;
            }
            const unsigned long long any_same = __ballot(act_same), any_mirror = __ballot(act_mirror);
            if ((any_same | any_mirror) == 0ull) continue;
            int d_same = INT32_MAX, d_mirror = INT32_MAX;
            if (any_same != 0ull) {
                const int score = distance_to_text<Word>(uniform<Word>(s_p0[jj]), uniform<Word>(s_p1[jj]), lb, la, top, eq0, eq1, eq2, eq3);
                if (act_same) d_same = score;
            }
            if (any_mirror != 0ull) {
                const int score = distance_to_text<Word>(uniform<Word>(s_m0[jj]), uniform<Word>(s_m1[jj]), lb, la, top, eq0, eq1, eq2, eq3);
                if (act_mirror) d_mirror = score;
            }
            const int d = min(d_same, d_mirror);
            const bool hit = d <= a.max_dist;            // (a lane active for neither holds INT32_MAX)
            const unsigned long long hits = __ballot(hit);
            if (hits != 0ull) {
                const int leader = __ffsll(hits) - 1;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(a.found, (unsigned long long)__popcll(hits));
                base = __shfl(base, leader);
                if (hit) {
                    const int64_t slot = (int64_t)(base + (unsigned long long)__popcll(hits & ((1ull << lane) - 1ull)));
                    if (slot < a.cap) {
                        int32_t *o = a.pairs + slot * 4;
                        o[0] = (int32_t)i;
                        o[1] = (int32_t)(J * kTile + jj);
                        o[2] = d;
                        o[3] = d_mirror < d_same ? 1 : 0;
                    }
                }
            }
        }
    }
}

}  // namespace

int launch_umi_neighbours_stranded(const UmiNeighboursArgs &a, void *stream)
{
    if (a.n < 2) return 0;
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    const int64_t total = tiles * (tiles + 1) / 2;
    const unsigned grid = (unsigned)std::min<int64_t>(total, (int64_t)1 << 20);      // the blocks stride over the rest
    if (a.max_len <= 32) hipLaunchKernelGGL(umi_neighbours_stranded_kernel<uint32_t>, dim3(grid), dim3(kTile), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(umi_neighbours_stranded_kernel<uint64_t>, dim3(grid), dim3(kTile), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_umi_neighbours(const UmiNeighboursArgs &a, void *stream)
{
    if (a.n < 2) return 0;
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    const int64_t total = tiles * (tiles + 1) / 2;
    const unsigned grid = (unsigned)std::min<int64_t>(total, (int64_t)1 << 20);      // the blocks stride over the rest
    if (a.max_len <= 32) hipLaunchKernelGGL(umi_neighbours_kernel<uint32_t>, dim3(grid), dim3(kTile), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(umi_neighbours_kernel<uint64_t>, dim3(grid), dim3(kTile), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace pck
