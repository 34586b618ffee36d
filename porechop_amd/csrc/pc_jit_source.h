// pc_jit_source.h -- source of the adapter-SPECIALISED score-only scan kernel, compiled at run
// time with hiprtc for one (adapter_lo, adapter_hi, scoring scheme) (pc_jit.cpp).
//
// Two things make it cheaper than the generic kernels' 9 packed ops per cell pair:
//
//  1. Adapter known at compile time.  The per-column substitution terms of the (few) distinct
//     letter pairs k that occur in the adapter pair are fetched once per column from an LDS table
//     indexed by the read byte, and every row's diagonal is ONE op, d = T_diag + S[COMBO[r]] with
//     a static register index (generic: 4 ops, because the adapter base of a row is data).
//
//  2. Drifting coordinates.  Every DP value X(rho, j) (rho = register row 1..R, j = column) is
//     kept as  X~ = X + (rho + jj) * eps - C,  eps = -gap_extend, jj = columns since the last
//     renormalisation, C a centring constant; T = M + gap_open is kept one step ahead,
//     T~ = T + (rho + jj + 1) * eps - C.  A gap extension moves one row or one column and costs
//     -eps, so in these coordinates it is free:
//         H~(rho,j) = max(H~(rho,j-1), T~(rho,j-1))          (no  H + e;  U[rho] holds H~(rho,j-1) entering column j --
//                                                             except on the fp16 fast path, point 3)
//         V~(rho,j) = max(V~(rho-1,j), T~(rho-1,j))          (no  V + e)
//         d~        = T~(rho-1,j-1) + S~,   S~ = sub - open + eps   (folded into the table)
//         M~        = max3(d~, H~, V~);     T~ = M~ + (open + eps)
//     5 packed ops per cell pair with fp16's 3-input max (v_pk_maximum3_f16), 6 with int16: the ONE-column path of both
//     lane types and the int16 column pair.  The packed-fp16 column pair (point 3) needs 4.75.  The
//     values are the same integers as the reference's, only offset by a known amount, so results
//     are bit-identical: row 0 (M = 0) becomes the per-column scalar `top`, the tracked last-row
//     score is T~(R,j) - top(j) = M(R,j) + R*eps, compared with strict '>' like dp_scout.h.
//     Values drift up by eps per column; every PC_KREN columns the state is shifted back down
//     (2R+1 ops per PC_KREN columns).  PC_KREN and C are chosen by the host so that every value
//     ever formed is an integer fp16 (|v| <= 2048) or int16 represents exactly (pc_jit.cpp).
//
//  3. Two columns per wave (column2 below, the block-resolved fast path): two dependency chains, column j and
//     column j+1 behind it, interleaved instruction by instruction instead of one chain padded with wait states.
//     Packed fp16: blocked 2 x 2, 19 ops per two rows and two columns = 4.75 per cell pair.  max is associative
//     and idempotent and the 3-input max costs one op, so H is materialised only every second column and V only
//     every second row:
//         Vb     = max3(Vb of the pair above, T~(e-2,.), T~(e-1,.))       V~ of the even row e of a row pair (e, o)
//         M(e,j)   = max3(d, U[e], Vb)                       M(o,j)   = max(max3(d, U[o], Vb), T~(e,j))
//         M(e,j+1) = max(max3(d', U[e], T~(e,j)), Vb')       M(o,j+1) = max3(max3(d', U[o], T~(o,j)), Vb', T~(e,j+1))
//         U[.]   = max3(U[.], T~(.,j), T~(.,j+1))                         once per column pair
//     11 maxima + 8 adds.  On this path U[rho] is ONE COLUMN AHEAD: it holds H~(rho, j) of the coming column j,
//     where the one-column path keeps H~(rho, j-1).  Entering the fast path converts, U = max(U, T), once per
//     entry; leaving it needs nothing, because the one-column path forms max(U, T), which is then U itself (the
//     same holds for the parked last-column state and for the renormalisation, which shifts T and U alike).
//     Every value formed is a maximum of values the five-op recurrence forms: same results, same range proof.
//     Chain B runs one row pair behind chain A; column j lives in registers of its own (X[]) for the two
//     statements until B has used it, so that every loop-carried T[r] keeps its register (see column2).
//     Packed int16 has no 3-input max: its column pair keeps six ops per cell pair, U = H~(rho, j-1), and the
//     skew of three rows.
//
// Padding rows (shorter adapter of a pair) use a letter whose substitution score is 0, which
// keeps M = 0 like row 0.  The kernel is score-only (pass 1 of the whole-read scan) and
// bit-identical in outputs to scan_kernel<R, *, false>; tests run both (PC_DISABLE_JIT=1 selects
// the generic one).
#pragma once

namespace pcj {

// defines prepended by pc_jit.cpp: PC_DUAL (1: the two adapters differ), PC_R, PC_K (multiple of 4), PC_COMBO_INIT (R comma-separated
// ints), PC_F16, PC_EPS (= -gap_extend), PC_OE (= gap_open + PC_EPS), PC_CEN (C), PC_KREN,
// PC_WAVES (resident waves per SIMD the register allocation must allow), PC_CHECK_RANGE (0/1); the row-skipping variant
// of a pair (a kernel of its own: pc_bounds.h row_skip_plan) also gets PC_R0, the register row it tests.
// PC_TOP=1 (with PC_MLO, PC_MHI, PC_KUP; only ever together with PC_R0): the row-skipping variant of a pair of different
// lengths, the shorter adapter TOP-aligned (pc_bounds.h row_skip_plan_top).  Register row = adapter row in both halves:
//   * column 0's lower-bound state "row-0 start + vertical gap" counts its rows from register row 1 in both halves;
//   * the tracked last row of a half is register row m_h -- PC_MLO / PC_MHI, compile-time constants, both below PC_R0 -- so the
//     tracked term is M(m_h, j) + m_h * eps, a packed select of two rows, formed by the one-column path and, while the lower
//     rows are on, by lower_block; packbest / unpack_best and every candidate term take m_h * eps per half;
//   * the last column's candidates are register rows 1 .. m_h of each half and never a row below m_h: the padding rows
//     below the shorter adapter hold real numbers (their letter scores 0 against everything, so they carry the maximum of
//     what lies above and to the left on), which may well exceed the real rows' -- nothing reads them, nothing takes them;
//   * those numbers stay inside spec_plan's range gate: a padding cell's M is at most the largest M of the real rows (0 is
//     added on the diagonal, gaps only cost), so <= match * R like every cell, and at least the in-column alternative "row-0
//     start + vertical gap" every cell has, which is what the gate's lower end is made of (the diagonal term 0 is >= the
//     gate's open + ext for a rewarded mismatch, >= mismatch otherwise); its register row is <= R like every row's;
//   * the rows above PC_R0 use the first PC_KUP letter pairs only (pc_jit.cpp numbers them in row order): the fast path
//     fetches PC_KUP terms per column, the lower part and the one-column path read the full row.
static const char *kSpecSource = R"PCJIT(
typedef unsigned int u32;
typedef long long i64;
#ifndef PC_TOP
#define PC_TOP 0
#endif
#if !PC_TOP
#define PC_MLO PC_R
#define PC_MHI PC_R
#define PC_KUP PC_K
#endif
#if PC_F16
// Packed FP16: every value formed is an integer with |v| <= 2048 (host-side gate), which fp16
// holds and adds exactly; -infinity is the real one.
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h16x2 SV(u32 x) { return __builtin_bit_cast(h16x2, x); }
__device__ __forceinline__ u32 WV(h16x2 x) { return __builtin_bit_cast(u32, x); }
__device__ __forceinline__ u32 pack2x(int l, int h) { const h16x2 v = {(_Float16)l, (_Float16)h}; return WV(v); }
__device__ __forceinline__ int lo16(u32 x) { return (int)(float)SV(x).x; }
__device__ __forceinline__ int hi16(u32 x) { return (int)(float)SV(x).y; }
#define PC_NEGBITS 0xFC00FC00u
#define PC_POSBITS 0x7C007C00u
#define PC_ADD "v_pk_add_f16"
#define PC_MAX "v_pk_max_f16"
#else
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 SV(u32 x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ u32 WV(s16x2 x) { return __builtin_bit_cast(u32, x); }
__device__ __forceinline__ u32 pack2x(int l, int h) { return ((u32)l & 0xFFFFu) | ((u32)h << 16); }
__device__ __forceinline__ int lo16(u32 x) { return (int)(short)(x & 0xFFFFu); }
__device__ __forceinline__ int hi16(u32 x) { return (int)(short)(x >> 16); }
#define PC_NEGBITS 0x80008000u
#define PC_POSBITS 0x7FFF7FFFu
#define PC_ADD "v_pk_add_u16"
#define PC_MAX "v_pk_max_i16"
#endif
__device__ __forceinline__ u32 pk_add(u32 a, u32 b) { return WV(SV(a) + SV(b)); }
__device__ __forceinline__ u32 pk_sub(u32 a, u32 b) { return WV(SV(a) - SV(b)); }
__device__ __forceinline__ u32 pk_max(u32 a, u32 b) { return WV(__builtin_elementwise_max(SV(a), SV(b))); }
__device__ __forceinline__ u32 pk_min(u32 a, u32 b) { return WV(__builtin_elementwise_min(SV(a), SV(b))); }
__device__ __forceinline__ u32 pack2(int v) { return pack2x(v, v); }
#if PC_F16
// IEEE-754-2019 maximum = v_pk_maximum3_f16: no canonicalising op on operands the compiler cannot prove quiet (never NaN here)
__device__ __forceinline__ u32 pk_maxq(u32 a, u32 b) { return WV(__builtin_elementwise_maximum(SV(a), SV(b))); }
#else
__device__ __forceinline__ u32 pk_maxq(u32 a, u32 b) { return pk_max(a, b); }
#endif
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 UV16(u32 x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ u32 WV16(u16x2 x) { return __builtin_bit_cast(u32, x); }
__device__ __forceinline__ u32 pk_minu(u32 a, u32 b) { return WV16(__builtin_elementwise_min(UV16(a), UV16(b))); }
__device__ __forceinline__ u32 pk_subu(u32 a, u32 b) { return WV16(UV16(a) - UV16(b)); }
__device__ __forceinline__ u32 pk_madu(u32 a, u32 k, u32 c) { return WV16(UV16(a) * UV16(k) + UV16(c)); }
// packed "best so far" in the tracked-score domain (score + R*eps; top-aligned: + m*eps of each half); the chunk>0 sentinel maps to -inf
__device__ __forceinline__ u32 packbest(int l, int h)
{
    const u32 v = pack2x(l > -20000 ? l + PC_MLO * PC_EPS : 0, h > -20000 ? h + PC_MHI * PC_EPS : 0);
    return (l > -20000 ? (v & 0xFFFFu) : (PC_NEGBITS & 0xFFFFu)) | (h > -20000 ? (v & 0xFFFF0000u) : (PC_NEGBITS & 0xFFFF0000u));
}

struct Tile { i64 win_lo, win_hi, out_lo, out_hi; int count_lo, count_hi, adapter_lo, adapter_hi, rows, pad_; };
struct SpecArgs {
    const unsigned char *arena; const i64 *win_off; const int *win_len;
    const Tile *tiles; int ntiles;
    int *out;                 // [npairs * chunks][4]: score, I, J, 0
    uint2 *fin_scratch;       // [grid][R][64]: row-major, lane fastest -- a store / load instruction of a wave is 512 contiguous bytes
    const u32 *s_table;       // [25 = code_lo * 5 + code_hi][PC_K]
    int m_lo, m_hi, gap_open, gap_extend;
    int chunks, chunk_len, span;
    u32 *err;
    u32 *work_counter;
    u32 one2;                 // 0x00010001, kept opaque to the compiler (with a literal it turns min_u16(x, 1) into compare / select chains)
    int *rec_out;             // score-only request over whole windows: [npairs][8] records (-2, J, I, 0, score, 0, 0, 0), else null
    const int *unit_prefix;   // [ntiles + 1] or null: tile t owns units [unit_prefix[t], unit_prefix[t + 1]) -- the chunks that hold columns
                              // of its longest window (a 4 Mb read among 20 kb reads: 2 048 chunks per tile, ten of them real for most)
    // row skip (pc_bounds.h row_skip_plan; floored two-pass calls only): skip_w = W_low > 0 switches it on; skip_thr2 = the packed
    // terms theta + r0 * eps - 1 of the two halves, which M(r0, j) + r0 * eps has to exceed for the rows below r0 to be computed
    u32 skip_thr2; int skip_w;
    unsigned long long *skip_count;   // null, or two counters: column pairs of the fast path, and those with the lower rows on
};
struct FastT { static constexpr bool fast = true; };
struct SlowT { static constexpr bool fast = false; };
template <int N> struct RowsT { static constexpr int rows = N; };
// PC_R0: the register row r0 the row skip tests (even, < PC_R), or PC_R: this kernel has no skipping path
#ifndef PC_R0
#define PC_R0 PC_R
#endif
#define PC_SKIP (PC_F16 && !PC_CHECK_RANGE && (PC_R0) < (PC_R))

__device__ static const unsigned char COMBO[PC_R] = { PC_COMBO_INIT };

typedef u32 u32_unaligned __attribute__((aligned(1)));

extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PC_WAVES))) void pc_spec_score(SpecArgs a)
{
    constexpr int R = PC_R, K = PC_K;
    // substitution terms by (code of the low stream's base, code of the high stream's base): 25 rows of K
    // packed terms, 1-4 KB instead of a row per byte value -- LDS no longer limits the waves per CU --
    // and the two bytes of a column reach their row through two small byte -> row-offset tables
    __shared__ uint4 s_tab[25 * K / 4];
    // (all three tables hold row offsets in BYTES, at most 24 * 16 * K / 4 < 2^16: a row's address is one add)
    __shared__ unsigned short lut_lo[256], lut_hi[256];
#if PC_SKIP
    __shared__ uint2 s_low[(PC_R - (PC_R0)) * 64];           // (T~, U) of the rows below r0 during a stretch of fast-path blocks (row skip)
#endif
#if PC_DUAL
    // two DIFFERENT adapters only ever share a tile whose halves read the same windows (pc_api.cpp
    // build_tiles): one byte stream per lane, and the byte -> table row lookup is a single read
    __shared__ unsigned short lut_one[256];                  // byte offset of row code * 6
#endif
    const int lane = threadIdx.x;
    for (int i = lane; i < 25 * K / 4; i += 64) s_tab[i] = ((const uint4 *)a.s_table)[i];
    for (int c = lane; c < 256; c += 64) {
        const int code = (c == 'A' || c == 'a') ? 0 : (c == 'C' || c == 'c') ? 1 : (c == 'G' || c == 'g') ? 2
                       : (c == 'T' || c == 't' || c == 'U' || c == 'u') ? 3 : 4;
        lut_lo[c] = (unsigned short)(code * 5 * (K / 4) * 16);
        lut_hi[c] = (unsigned short)(code * (K / 4) * 16);
#if PC_DUAL
        lut_one[c] = (unsigned short)(code * 6 * (K / 4) * 16);
#endif
    }
    __syncthreads();
    const u32 OE2 = pack2(PC_OE), EPS2 = pack2(PC_EPS), NEG2 = PC_NEGBITS;
    const int pad_lo = PC_TOP ? 0 : R - a.m_lo, pad_hi = PC_TOP ? 0 : R - a.m_hi;   // (top-aligned: no padding above)
    // previous-column state of the lanes whose read ends (one region per half: in a tile of two read
    // streams the halves of a lane end in different columns)
    uint2 *fin = a.fin_scratch + (i64)blockIdx.x * 2 * R * 64;
    uint2 *fin_hi_buf = fin + (PC_DUAL ? 0 : R * 64);
    const int nchunks = a.chunks > 1 ? a.chunks : 1;

    // Units (tile x column chunk) are taken in launch order -- the host hands tiles over longest first -- the
    // first gridDim.x by the hardware dispatcher, the rest from a counter: a workgroup that drew short units
    // simply draws more of them, so reads of very different lengths still fill the chip to the end.
    auto next_unit = [&](int vt) -> int {
        if (!a.work_counter) return vt + (int)gridDim.x;
        u32 v = 0;
        if (lane == 0) v = atomicAdd(a.work_counter, 1u);
        return (int)gridDim.x + (int)__builtin_amdgcn_readfirstlane(v);
    };
    const int total_units = a.unit_prefix ? a.unit_prefix[a.ntiles] : a.ntiles * nchunks;
    for (int vt = blockIdx.x; vt < total_units; vt = next_unit(vt)) {
        int t, chunk;
        if (a.unit_prefix) {                                     // the last tile whose first unit is <= vt (wave-uniform)
            int lo = 0, hi = a.ntiles - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.unit_prefix[mid] <= vt) lo = mid; else hi = mid - 1; }
            t = lo; chunk = vt - a.unit_prefix[lo];
        } else {
            t = vt / nchunks; chunk = vt - t * nchunks;
        }
        const Tile tile = a.tiles[t];
#if PC_DUAL
        constexpr bool one_stream = true;
        if (tile.win_lo != tile.win_hi) {                        // host bug
            if (lane == 0) atomicAdd(a.err, 1u);
            continue;
        }
#else
        const bool one_stream = tile.win_lo == tile.win_hi;
#endif
        const i64 p_lo = tile.out_lo + lane, p_hi = tile.out_hi + lane;
        const bool have_lo = lane < tile.count_lo, have_hi = lane < tile.count_hi;
        const unsigned char *w_lo = a.arena + (have_lo ? a.win_off[tile.win_lo + lane] : 0);
        const unsigned char *w_hi = a.arena + (have_hi ? a.win_off[tile.win_hi + lane] : 0);
        int n_lo = have_lo ? a.win_len[tile.win_lo + lane] : 0;
        int n_hi = have_hi ? a.win_len[tile.win_hi + lane] : 0;
        int c0_lo = 0, c0_hi = 0, tf_lo = 0, tf_hi = 0;
        bool tail_lo = true, tail_hi = true;
        if (nchunks > 1) {
            const int L = a.chunk_len, start = chunk * L;
            auto cut = [&](int nfull, const unsigned char *&w, int &n, int &c0, int &tf, bool &tail) {
                if (start >= nfull) { n = 0; c0 = 0; tf = 0; tail = false; return; }
                c0 = start - a.span > 0 ? start - a.span : 0;
                const int end = start + L < nfull ? start + L : nfull;
                w += c0; n = end - c0; tf = start - c0; tail = (end == nfull);
            };
            cut(n_lo, w_lo, n_lo, c0_lo, tf_lo, tail_lo);
            cut(n_hi, w_hi, n_hi, c0_hi, tf_hi, tail_hi);
        }
        // column 0: M = 0 (T = open) for a window at the read's column 0, otherwise the lower-bound
        // state "row-0 start + vertical gap" (see pc_bounds.h); drifting coordinates with jj = 0
        u32 T[R], U[R];
#pragma clang loop unroll(full)
        for (int r = 0; r < R; ++r) {
            const int vl = (c0_lo > 0 && r >= pad_lo) ? 2 * a.gap_open + (r - pad_lo) * a.gap_extend : a.gap_open;
            const int vh = (c0_hi > 0 && r >= pad_hi) ? 2 * a.gap_open + (r - pad_hi) * a.gap_extend : a.gap_open;
            T[r] = pack2x(vl + (r + 2) * PC_EPS - PC_CEN, vh + (r + 2) * PC_EPS - PC_CEN);
            U[r] = NEG2;
        }
        u32 top = pack2(a.gap_open + PC_EPS - PC_CEN);      // T~(0, j-1) entering column j
        int bs_lo = 0, bi_lo = a.m_lo, bj_lo = 0, bs_hi = 0, bi_hi = a.m_hi, bj_hi = 0;
        if (chunk > 0) { bs_lo = -32768; bj_lo = -1; bs_hi = -32768; bj_hi = -1; }   // (m,0) belongs to chunk 0
        u32 best2 = packbest(bs_lo, bs_hi);
        u32 ftop = 0;                                       // T~(0, n-1) of each half when its read ended
        // In the block-resolved path the running maximum and its column live PACKED (best2: the tracked
        // score term, pos2: the column as two u16; 0xFFFF = none yet): a new maximum costs five packed ops
        // per column for both halves instead of two conversions and two compare / select chains.  The int
        // copies (bs, bj) are brought up to date where the per-stream path or the output needs them.
        u32 pos2 = ((u32)bj_lo & 0xFFFFu) | ((u32)bj_hi << 16);
        bool packed_ahead = false;                          // wave-uniform: (best2, pos2) are newer than (bs, bj)
        auto unpack_best = [&]() {
            bs_lo = ((best2 & 0xFFFFu) == (PC_NEGBITS & 0xFFFFu)) ? -32768 : lo16(best2) - PC_MLO * PC_EPS;
            bs_hi = ((best2 >> 16) == (PC_NEGBITS >> 16)) ? -32768 : hi16(best2) - PC_MHI * PC_EPS;
            bj_lo = ((pos2 & 0xFFFFu) == 0xFFFFu) ? -1 : (int)(pos2 & 0xFFFFu);
            bj_hi = ((pos2 >> 16) == 0xFFFFu) ? -1 : (int)(pos2 >> 16);
            bi_lo = a.m_lo; bi_hi = a.m_hi;                 // every cell tracked inside the column loop is a last-row cell
            packed_ahead = false;
        };
        const u32 ONE2 = a.one2;
        // wave-uniform extents: columns in (tfmax, nmin) are tracked by every stream of the tile
        int nmax = n_lo > n_hi ? n_lo : n_hi;
        int nmin = have_lo ? n_lo : 0x7FFFFFFF;
        if (have_hi && n_hi < nmin) nmin = n_hi;
        int tfmax = tf_lo > tf_hi ? tf_lo : tf_hi;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            int o = __shfl_xor(nmax, s); nmax = o > nmax ? o : nmax;
            o = __shfl_xor(nmin, s); nmin = o < nmin ? o : nmin;
            o = __shfl_xor(tfmax, s); tfmax = o > tfmax ? o : tfmax;
        }
#if PC_SKIP
        // (the extents are wave-uniform, but come out of a shuffle: said so, the fast path's tests and the window's state
        // below are scalar branches and scalar registers, not exec masks and copies of every row's registers)
        nmax = __builtin_amdgcn_readfirstlane(nmax); nmin = __builtin_amdgcn_readfirstlane(nmin); tfmax = __builtin_amdgcn_readfirstlane(tfmax);
#endif
        // Every stream of the tile ends in the SAME column (equal-length windows: the 150-column end windows of phase B's
        // score pass, the uniform reads of the benchmark): the column loop then stops exactly there and the last column's
        // cells are scanned straight from the registers.  Otherwise (ragged tiles) a lane that ends parks the state its last
        // column starts from in fin_scratch and the column is re-run from there after the loop.  (The parked state costs
        // R*64*8 B per half and tile, out and back in: 37 GB per step of a 196-job phase B, for nothing.)
        const bool uniform_fin = nmax > 0 && nmin == nmax && __all((!have_lo || tail_lo) && (!have_hi || tail_hi));

        // Read bytes are fetched 16 columns at a time into q_lo / q_hi and handed to the column loop a dword
        // (4 columns) at a time, one dword ahead; the substitution terms S[] of column j+1 are fetched from
        // the LDS table while column j computes (two register sets, the column loop statically unrolled by
        // 4), so neither the global load nor the LDS read latency sits on the column's critical path.
        // Why 16 bytes: every lane reads its own window, so a load instruction touches 64 (two streams: 128)
        // different cache lines, and the lines a CU's waves have open (12 waves x 128 x 128 B) are far more
        // than its L1 holds -- each load is an L2 request per lane.  With a dword per load a tile of two read
        // streams asked L2 for 32 x the bytes it used and ran at a third of the one-stream tiles' rate
        // (measured, 150-column windows: 3.6 vs 9.8 TCUPS); 16 bytes per load is a quarter of the requests.
        auto load_q = [&](const unsigned char *w, int n, int col) -> uint4 {   // the 16 columns from 0-based column col
            const int k = (col < n) ? col : (n > 0 ? ((n - 1) & ~15) : 0);     // finished streams re-read their last block
            uint4 v;
            __builtin_memcpy(&v, w + k, 16);                                   // any alignment: one global_load_dwordx4
            return v;
        };
        auto pick_dw = [&](const uint4 &q, int k) -> u32 {                     // k is wave-uniform
            return k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w;
        };
#if PC_CHECK_RANGE
        // debug build (PC_JIT_CHECK_RANGE=1): every column takes the one-column path and the extremes of EVERY value
        // formed are recorded -- the column state T / U after each column, every row's diagonal term d and vertical
        // state V (the cell maximum M is one of d, H, V; the new T is recorded with the state), the top-row term, the
        // tracked last-row term the scout compares, the last-column re-run's values -- the host-side range gate
        // (pc_bounds.h spec_plan) asserted on the device.  (The substitution-table terms are bounded on the host, where
        // the table is built: pc_jit.cpp.)  The "-infinity" a column's H / V start from is absorbed by the first max.
        u32 vmax = PC_NEGBITS, vmin = PC_POSBITS;
#define PC_NOTE_V(x) { vmax = pk_max(vmax, (x)); vmin = pk_min(vmin, (x)); }
#else
#define PC_NOTE_V(x)
#endif
        auto fetch_Sn = [&](auto up, u32 (&S)[K], u32 bl, u32 bh) {
            constexpr bool UP = decltype(up)::fast;
#if PC_DUAL
            const uint4 *row = (const uint4 *)((const char *)s_tab + (u32)lut_one[bl]);
#else
            const uint4 *row = (const uint4 *)((const char *)s_tab + ((u32)lut_lo[bl] + (u32)lut_hi[one_stream ? bl : bh]));
#endif
#pragma clang loop unroll(full)
            for (int q = 0; q < (UP ? PC_KUP : K) / 4; ++q) { const uint4 v = row[q]; S[4*q] = v.x; S[4*q+1] = v.y; S[4*q+2] = v.z; S[4*q+3] = v.w; }
        };
        auto fetch_S = [&](u32 (&S)[K], u32 bl, u32 bh) { fetch_Sn(SlowT{}, S, bl, bh); };
        // the terms of the rows above r0 only (row skip, top-aligned: the first PC_KUP letter pairs)
        auto fetch_S_up = [&](u32 (&S)[K], u32 bl, u32 bh) { fetch_Sn(FastT{}, S, bl, bh); };
        // One column.  Returns the tracked last-row term T~(R,j) - top(j) = M(R,j) + R*eps.
        // FastT: every stream of the tile tracks this column and none ends in it (the caller
        // resolves maxima per 4-column block); SlowT: per-stream masks, last-column handling.
        auto column = [&](auto tag, const int j, const u32 (&S)[K]) -> u32 {
            constexpr bool FAST = decltype(tag)::fast;
            bool fin_lo = false, fin_hi = false, any_fin = false;
            if constexpr (!FAST) {
                // A read's LAST column is scanned row by row (every cell of it is an end candidate,
                // dp_scout.h:165-179) -- after the column loop, for all lanes of the tile at once: here the
                // lanes that end in this column only park the state the column starts from.
                fin_lo = (j == n_lo) && tail_lo && !uniform_fin; fin_hi = (j == n_hi) && tail_hi && !uniform_fin;
                any_fin = __any(fin_lo || fin_hi);
                if (any_fin) {
                    if (fin_lo) {
#pragma clang loop unroll(full)
                        for (int r = 0; r < R; ++r) fin[r * 64 + lane] = make_uint2(T[r], U[r]);
                    }
#if !PC_DUAL
                    if (fin_hi) {
#pragma clang loop unroll(full)
                        for (int r = 0; r < R; ++r) fin_hi_buf[r * 64 + lane] = make_uint2(T[r], U[r]);
                    }
#endif
                    ftop = (fin_lo ? (top & 0xFFFFu) : (ftop & 0xFFFFu)) | (fin_hi ? (top & 0xFFFF0000u) : (ftop & 0xFFFF0000u));
                }
            }
            const u32 topn = pk_add(top, EPS2);               // T~(0, j)
            // ---- the column, hand-scheduled.  gfx950 needs a wait state between dependent packed
            // ops; each row's serial chain (V, M, T') is interleaved with row r+2's independent half
            // (H in place into U[q], d into dh[q]); the one gap nothing can fill is an s_nop,
            // which the other waves of the SIMD use.
            {
                constexpr int KP = 2;
                u32 dh[R];     // d of the rows in flight
                auto ind_only = [&](int q, u32 diag) {
                    asm volatile(PC_MAX " %[uq], %[uq], %[tq]\n\t"
                                 PC_ADD " %[dq], %[diag], %[s]"
                                 : [dq] "=&v"(dh[q]), [uq] "+v"(U[q])
                                 : [diag] "v"(diag), [s] "v"(S[COMBO[q]]), [tq] "v"(T[q]));
                };
#pragma clang loop unroll(full)
                for (int q = 0; q < KP && q < R; ++q) ind_only(q, q == 0 ? top : T[q - 1]);
                u32 Tup = topn, Vprev = NEG2;
#if PC_F16
                // 5 ops: H' (in place), V, d', M = max3(d, H, V), T      (primed = row r+2)
#define PC_ROW_FULL(VP, TU, DIAG, SS, UQ, TQ, DHR, UR, TN, DHQ, VS)                  \
    PC_MAX " " UQ ", " UQ ", " TQ "\n\t"                                              \
    PC_MAX " " VS ", " VP ", " TU "\n\t"                                              \
    PC_ADD " " DHQ ", " DIAG ", " SS "\n\t"                                           \
    "v_pk_maximum3_f16 %[mn], " DHR ", " UR ", " VS "\n\t"                            \
    "s_nop 0\n\t"                                                                     \
    PC_ADD " " TN ", %[mn], %[oe]\n\t"
#define PC_ROW_TAIL                                                                    \
    "s_nop 0\n\t"                                                                      \
    PC_MAX " %[vs0], %[vprev], %[tup]\n\t" "s_nop 0\n\t"                               \
    "v_pk_maximum3_f16 %[mn], %[dhr0], %[ur0], %[vs0]\n\t" "s_nop 0\n\t"               \
    PC_ADD " %[tn0], %[mn], %[oe]"
#else
                // 6 ops: max(d,H), H' (in place), V, d', M = max(max(d,H), V), T
#define PC_ROW_FULL(VP, TU, DIAG, SS, UQ, TQ, DHR, UR, TN, DHQ, VS)                  \
    PC_MAX " %[mn], " DHR ", " UR "\n\t"                                              \
    PC_MAX " " UQ ", " UQ ", " TQ "\n\t"                                              \
    PC_MAX " " VS ", " VP ", " TU "\n\t"                                              \
    PC_ADD " " DHQ ", " DIAG ", " SS "\n\t"                                           \
    PC_MAX " %[mn], %[mn], " VS "\n\t"                                                \
    "s_nop 0\n\t"                                                                     \
    PC_ADD " " TN ", %[mn], %[oe]\n\t"
#define PC_ROW_TAIL                                                                    \
    PC_MAX " %[mn], %[dhr0], %[ur0]\n\t"                                               \
    PC_MAX " %[vs0], %[vprev], %[tup]\n\t" "s_nop 0\n\t"                               \
    PC_MAX " %[mn], %[mn], %[vs0]\n\t" "s_nop 0\n\t"                                   \
    PC_ADD " %[tn0], %[mn], %[oe]"
#endif
#pragma clang loop unroll(full)
                for (int r = 0; r < R; r += 2) {
                    u32 mn, vs0, vs1;
                    if (r + 1 + KP < R) {
                        const int q = r + KP;
                        // row q's diagonal is T[q - 1] = T[r + 1], which this statement also produces (its last instruction,
                        // after the read): ONE in-out operand, so the register is updated in place.  As a separate input
                        // beside an early-clobber output it cost a copy per row pair -- and the first column's copies were
                        // hoisted above the branch, into the block-resolved path (profiles/score_block_audit.txt)
                        static_assert(KP == 2, "the tied operand below is T[q - 1] = T[r + 1]");
                        asm volatile(
                            PC_ROW_FULL("%[vprev]", "%[tup]", "%[tn1]", "%[s0]", "%[u0]", "%[t0]", "%[dhr0]", "%[ur0]", "%[tn0]", "%[dhq0]", "%[vs0]")
                            PC_ROW_FULL("%[vs0]", "%[tn0]", "%[t0]", "%[s1]", "%[u1]", "%[t1]", "%[dhr1]", "%[ur1]", "%[tn1]", "%[dhq1]", "%[vs1]")
                            : [mn] "=&v"(mn), [vs0] "=&v"(vs0), [vs1] "=&v"(vs1),
                              [u0] "+v"(U[q]), [u1] "+v"(U[q + 1]), [tn0] "=&v"(T[r]), [tn1] "+v"(T[r + 1]),
                              [dhq0] "=&v"(dh[q]), [dhq1] "=&v"(dh[q + 1])
                            : [vprev] "v"(Vprev), [tup] "v"(Tup), [oe] "s"(OE2),
                              [t0] "v"(T[q]), [t1] "v"(T[q + 1]), [s0] "v"(S[COMBO[q]]), [s1] "v"(S[COMBO[q + 1]]),
                              [dhr0] "v"(dh[r]), [dhr1] "v"(dh[r + 1]), [ur0] "v"(U[r]), [ur1] "v"(U[r + 1]));
                        PC_NOTE_V(dh[r]) PC_NOTE_V(dh[r + 1]) PC_NOTE_V(vs0) PC_NOTE_V(vs1)
                        Tup = T[r + 1]; Vprev = vs1;
                    } else {
                        // tail rows (and an odd last row): one row at a time
#pragma clang loop unroll(full)
                        for (int rr = r; rr < r + 2 && rr < R; ++rr) {
                            if (rr + KP < R) {
                                const int q = rr + KP;
                                asm volatile(
                                    PC_ROW_FULL("%[vprev]", "%[tup]", "%[d0]", "%[s0]", "%[u0]", "%[t0]", "%[dhr0]", "%[ur0]", "%[tn0]", "%[dhq0]", "%[vs0]")
                                    : [mn] "=&v"(mn), [vs0] "=&v"(vs0),
                                      [u0] "+v"(U[q]), [tn0] "=&v"(T[rr]), [dhq0] "=&v"(dh[q])
                                    : [vprev] "v"(Vprev), [tup] "v"(Tup), [oe] "s"(OE2), [d0] "v"(T[q - 1]),
                                      [t0] "v"(T[q]), [s0] "v"(S[COMBO[q]]), [dhr0] "v"(dh[rr]), [ur0] "v"(U[rr]));
                            } else {
                                asm volatile(PC_ROW_TAIL
                                             : [vs0] "=&v"(vs0), [mn] "=&v"(mn), [tn0] "=&v"(T[rr])
                                             : [vprev] "v"(Vprev), [tup] "v"(Tup), [dhr0] "v"(dh[rr]),
                                               [ur0] "v"(U[rr]), [oe] "s"(OE2));
                            }
                            PC_NOTE_V(dh[rr]) PC_NOTE_V(vs0)
                            Tup = T[rr]; Vprev = vs0;
                        }
                    }
                }
#undef PC_ROW_FULL
#undef PC_ROW_TAIL
            }
#if PC_TOP
            const u32 cand = pk_sub((T[PC_MLO - 1] & 0xFFFFu) | (T[PC_MHI - 1] & 0xFFFF0000u), topn);   // each half's own last row
#else
            const u32 cand = pk_sub(T[R - 1], topn);
#endif
            PC_NOTE_V(cand) PC_NOTE_V(topn)
            if constexpr (!FAST) {
                const int cl = lo16(cand) - PC_MLO * PC_EPS, ch = hi16(cand) - PC_MHI * PC_EPS;
                const bool tr_lo = j > tf_lo && (tail_lo ? j < n_lo : j <= n_lo);
                const bool tr_hi = j > tf_hi && (tail_hi ? j < n_hi : j <= n_hi);
                if (tr_lo && cl > bs_lo) { bs_lo = cl; bi_lo = a.m_lo; bj_lo = j; }
                if (tr_hi && ch > bs_hi) { bs_hi = ch; bi_hi = a.m_hi; bj_hi = j; }
            }
            top = topn;
            return cand;
        };

#if PC_F16
        // Two columns at once, blocked 2 x 2: 19 packed ops per two rows and two columns instead of 20.
        // max is associative and idempotent and v_pk_maximum3_f16 takes three inputs for the price of one op,
        // so H is materialised only every second column and V only every second row:
        //   * U[r] holds H~(rho, j) of the coming EVEN column j (the one-column path: H~(rho, j-1)), and is
        //     brought up to date once per column pair, U = max3(U, T(., j), T(., j+1));
        //   * Vb is the V~ of the even row of a row pair, Vb = max3(Vb of the pair above, T(e-2, .), T(e-1, .)).
        // Per row pair (e, o) and column pair (j, j+1), chain A = column j, chain B = column j+1:
        //   A  Vb = max3(Vb, T(e-2,j), T(e-1,j))        M(e,j)   = max3(d, U[e], Vb)
        //                                               M(o,j)   = max(max3(d, U[o], Vb), T(e,j))
        //   B  Vb' = max3(Vb', T(e-2,j+1), T(e-1,j+1))  M(e,j+1) = max(max3(d', U[e], T(e,j)), Vb')
        //                                               M(o,j+1) = max3(max3(d', U[o], T(o,j)), Vb', T(e,j+1))
        //      U[e] = max3(U[e], T(e,j), T(e,j+1));  U[o] likewise
        // 11 maxima + 4 d + 4 T = 19 ops; the dependent chain per row pair and column is 5 ops (Vb, M, T, M, T).
        // Every value formed is a maximum of values the one-column recurrence forms, so results and the range
        // proof (pc_bounds.h spec_plan) are unchanged.  An odd last row runs as an even-type row on its own.
        //
        // Chain B runs ONE row pair behind chain A.  Each asm statement carries a row pair of A and the pair
        // above it of B, interleaved instruction by instruction so that no op reads the result of the op
        // before it: no s_nop in the steady state.  Registers: the U update reads T(., j) and T(., j+1)
        // together, so column j cannot be formed in place.  A writes it to X[] -- short-lived, a row's X dies
        // two statements later -- and T[r] goes T(r, j-1) -> d'(r) -> T(r, j+1) in ONE register: B forms
        // its diagonal term for row r in T[r] as soon as A has read the old value (an in-out operand, read
        // by A's d and then written), and its new T in place of that term.  Every loop-carried value thus
        // keeps its register from column pair to column pair and the allocator has nothing to rotate.
        // Only for blocks in which every stream of the tile tracks the columns and none ends (the caller's
        // fast path, which converts U on entry).
        //
        // Row skip (PC_SKIP, a launch with skip_w > 0): the column pair runs over the upper r0 = PC_R0 rows only and
        // leaves what the rows below need of row r0 -- if_va = V~(r0 - 1, j) (register rows: the even row of the last pair),
        // if_x0 / if_x1 = T~(r0 - 1, j) / T~(r0, j), if_vb = V~(r0 - 1, j + 1); T~(., j + 1) is in T[] -- see lower_col.
        u32 if_x0 = NEG2, if_x1 = NEG2, if_va = NEG2, if_vb = NEG2;
        auto column2 =[&](auto rows, const u32 (&S1)[K], const u32 (&S2)[K], u32 &c1, u32 &c2) {
            constexpr int RU = decltype(rows)::rows;                           // the rows it runs over: R, or the upper r0 (row skip)
            constexpr int NU = (RU + 1) / 2;                                    // units: row pairs, then an odd last row alone
            const u32 topA = pk_add(top, EPS2), topB = pk_add(topA, EPS2);     // T~(0,j), T~(0,j+1)
            u32 X[R], dA[R];                                                   // column j; chain A's d of the rows in flight
#define PC_M3 "v_pk_maximum3_f16"
#define PC_NOP "s_nop 0\n\t"
            // chain A: Vb, M(e), d(e+2), T(e), x(o), M(o), T(o), d(e+3)       (ta0 / ta1 = X[e] / X[o]; to1 / ta2 = T(o, j-1) / T(e+2, j-1);
            // beside chain B, T(o, j-1) is B's in-out operand db3: PC_A7I)
#define PC_A1 PC_M3 " %[va], %[vpa], %[tf], %[tg]\n\t"
#define PC_A2 PC_M3 " %[ta0], %[da0], %[ua0], %[va]\n\t"
#define PC_A7 PC_ADD " %[da2], %[to1], %[sa2]\n\t"
#define PC_A7I PC_ADD " %[da2], %[db3], %[sa2]\n\t"
#define PC_A3 PC_ADD " %[ta0], %[ta0], %[oe]\n\t"
#define PC_A4 PC_M3 " %[ta1], %[da1], %[ua1], %[va]\n\t"
#define PC_A5 PC_MAX " %[ta1], %[ta1], %[ta0]\n\t"
#define PC_A6 PC_ADD " %[ta1], %[ta1], %[oe]\n\t"
#define PC_A8 PC_ADD " %[da3], %[ta2], %[sa3]\n\t"
            // chain B: Vb', y(e), M(e), T(e), z(o), M(o), T(o), U[e], U[o], d'(e+2), d'(e+3)   (tb0 / tb1 = T[e] / T[o], which enter as
            // d'(e) / d'(o); tf / tg = X[e] / X[o]; db2 / db3 = T[e+2] / T[e+3])
#define PC_B1 PC_M3 " %[vb], %[vpb], %[tbm2], %[tbm1]\n\t"
#define PC_B2 PC_M3 " %[tb0], %[tb0], %[ub0], %[tf]\n\t"
#define PC_B3 PC_MAX " %[tb0], %[tb0], %[vb]\n\t"
#define PC_B4 PC_ADD " %[tb0], %[tb0], %[oe]\n\t"
#define PC_B5 PC_M3 " %[tb1], %[tb1], %[ub1], %[tg]\n\t"
#define PC_B6 PC_M3 " %[tb1], %[tb1], %[vb], %[tb0]\n\t"
#define PC_B7 PC_ADD " %[tb1], %[tb1], %[oe]\n\t"
#define PC_B8 PC_M3 " %[ub0], %[ub0], %[tf], %[tb0]\n\t"
#define PC_B9 PC_M3 " %[ub1], %[ub1], %[tg], %[tb1]\n\t"
#define PC_B10 PC_ADD " %[db2], %[tg], %[sb2]\n\t"
            // a pair of A with the pair above it of B; D2 / D3: A's look-ahead terms d(e+2) / d(e+3), where those rows exist
            // (B's d'(e+3) reads the T(e+2, j) = ta0 that A forms in this statement)
#define PC_AB(D2, D3)                                                                  \
    PC_A1 PC_B1 PC_A2 PC_B2 D2 PC_B3 PC_A3 PC_B4 PC_A4 PC_B5 PC_A5 PC_B6 PC_A6 PC_B8  \
    D3 PC_B7 PC_B10 PC_ADD " %[db3], %[ta0], %[sb3]\n\t" PC_B9
            // the odd last row of A with the last pair of B
#define PC_AB_ODD                                                                      \
    PC_A1 PC_B1 PC_A2 PC_B2 PC_B5 PC_B3 PC_A3 PC_B4 PC_B10 PC_B6 PC_B8 PC_B7 PC_NOP PC_B9
            // one chain on its own: A's first unit, B's last
#define PC_A_PAIR(D2, D3) D2 PC_A1 D3 PC_A2 PC_A4 PC_A3 PC_NOP PC_A5 PC_NOP PC_A6
#define PC_A_ODD PC_A1 PC_NOP PC_A2 PC_NOP PC_A3
#define PC_B_PAIR PC_B2 PC_B1 PC_B5 PC_B3 PC_NOP PC_B4 PC_NOP PC_B6 PC_B8 PC_B7 PC_NOP PC_B9
#define PC_B_ODD PC_B2 PC_B1 PC_NOP PC_B3 PC_NOP PC_B4 PC_NOP PC_B8
            auto dterm = [&](u32 &d, u32 diag, u32 s) { asm volatile(PC_ADD " %[d], %[g], %[s]" : [d] "=v"(d) : [g] "v"(diag), [s] "v"(s)); };
            u32 VbA = NEG2, VbB = NEG2, vbl = NEG2;
            // ---- chain A alone: its first unit (rows 0 and 1); T(-2, .) = -infinity, T(-1, .) = the top row
            dterm(dA[0], top, S1[COMBO[0]]);
            if constexpr (RU > 1) dterm(dA[1], T[0], S1[COMBO[1]]);
            {
                u32 va;
                if constexpr (RU >= 4) {
                    asm volatile(PC_A_PAIR(PC_A7, PC_A8)
                                 : [va] "=&v"(va), [ta0] "=&v"(X[0]), [ta1] "=&v"(X[1]), [da2] "=&v"(dA[2]), [da3] "=&v"(dA[3])
                                 : [vpa] "v"(VbA), [tf] "v"(NEG2), [tg] "v"(topA), [oe] "s"(OE2), [da0] "v"(dA[0]), [da1] "v"(dA[1]),
                                   [ua0] "v"(U[0]), [ua1] "v"(U[1]), [to1] "v"(T[1]), [sa2] "v"(S1[COMBO[2]]), [sa3] "v"(S1[COMBO[3]]), [ta2] "v"(T[2]));
                } else if constexpr (RU == 3) {
                    asm volatile(PC_A_PAIR(PC_A7, PC_NOP)
                                 : [va] "=&v"(va), [ta0] "=&v"(X[0]), [ta1] "=&v"(X[1]), [da2] "=&v"(dA[2])
                                 : [vpa] "v"(VbA), [tf] "v"(NEG2), [tg] "v"(topA), [oe] "s"(OE2), [da0] "v"(dA[0]), [da1] "v"(dA[1]),
                                   [ua0] "v"(U[0]), [ua1] "v"(U[1]), [to1] "v"(T[1]), [sa2] "v"(S1[COMBO[2]]));
                } else if constexpr (RU == 2) {
                    asm volatile(PC_A_PAIR("", PC_NOP)
                                 : [va] "=&v"(va), [ta0] "=&v"(X[0]), [ta1] "=&v"(X[1])
                                 : [vpa] "v"(VbA), [tf] "v"(NEG2), [tg] "v"(topA), [oe] "s"(OE2), [da0] "v"(dA[0]), [da1] "v"(dA[1]),
                                   [ua0] "v"(U[0]), [ua1] "v"(U[1]));
                } else {
                    asm volatile(PC_A_ODD
                                 : [va] "=&v"(va), [ta0] "=&v"(X[0])
                                 : [vpa] "v"(VbA), [tf] "v"(NEG2), [tg] "v"(topA), [oe] "s"(OE2), [da0] "v"(dA[0]), [ua0] "v"(U[0]));
                }
                VbA = va;
            }
            // ---- chain B starts: its rows 0 and 1 read column j's top row and T(0), which A has produced
            // (its d' go where the rows' old T was: in-out, so that the register stays the row's)
            auto dterm_b = [&](u32 &t, u32 diag, u32 s) { asm volatile(PC_ADD " %[t], %[g], %[s]" : [t] "+v"(t) : [g] "v"(diag), [s] "v"(s)); };
            dterm_b(T[0], topA, S2[COMBO[0]]);
            if constexpr (RU > 1) dterm_b(T[1], X[0], S2[COMBO[1]]);
#pragma clang loop unroll(full)
            for (int u = 1; u < NU; ++u) {
                const int e = 2 * u, f = e - 2;                                // A: rows e, e+1; B: rows f, f+1
                const u32 tbm2 = f ? T[f - 2] : NEG2, tbm1 = f ? T[f - 1] : topB;
                u32 va, vb;
#define PC_AB_OUT  [va] "=&v"(va), [vb] "=&v"(vb), [ta0] "=&v"(X[e]), [tb0] "+v"(T[f]), [tb1] "+v"(T[f + 1]), \
                   [ub0] "+v"(U[f]), [ub1] "+v"(U[f + 1]), [db2] "+v"(T[e])
#define PC_AB_IN   [vpa] "v"(VbA), [vpb] "v"(VbB), [tbm2] "v"(tbm2), [tbm1] "v"(tbm1), [tf] "v"(X[f]), [tg] "v"(X[f + 1]), \
                   [oe] "s"(OE2), [da0] "v"(dA[e]), [ua0] "v"(U[e]), [sb2] "v"(S2[COMBO[f + 2]])
                if (e + 3 < RU) {
                    asm volatile(PC_AB(PC_A7I, PC_A8)
                                 : PC_AB_OUT, [ta1] "=&v"(X[e + 1]), [db3] "+v"(T[e + 1]), [da2] "=&v"(dA[e + 2]), [da3] "=&v"(dA[e + 3])
                                 : PC_AB_IN, [da1] "v"(dA[e + 1]), [ua1] "v"(U[e + 1]), [sb3] "v"(S2[COMBO[f + 3]]),
                                   [sa2] "v"(S1[COMBO[e + 2]]), [sa3] "v"(S1[COMBO[e + 3]]), [ta2] "v"(T[e + 2]));
                } else if (e + 2 < RU) {
                    asm volatile(PC_AB(PC_A7I, "")
                                 : PC_AB_OUT, [ta1] "=&v"(X[e + 1]), [db3] "+v"(T[e + 1]), [da2] "=&v"(dA[e + 2])
                                 : PC_AB_IN, [da1] "v"(dA[e + 1]), [ua1] "v"(U[e + 1]), [sb3] "v"(S2[COMBO[f + 3]]),
                                   [sa2] "v"(S1[COMBO[e + 2]]));
                } else if (e + 1 < RU) {
                    asm volatile(PC_AB(PC_NOP, "")
                                 : PC_AB_OUT, [ta1] "=&v"(X[e + 1]), [db3] "+v"(T[e + 1])
                                 : PC_AB_IN, [da1] "v"(dA[e + 1]), [ua1] "v"(U[e + 1]), [sb3] "v"(S2[COMBO[f + 3]]));
                } else {
                    asm volatile(PC_AB_ODD : PC_AB_OUT : PC_AB_IN);
                }
#undef PC_AB_OUT
#undef PC_AB_IN
                VbA = va; VbB = vb;
            }
            c1 = pk_sub(X[RU - 1], topA);               // column j's last row
            // ---- chain B alone: its last unit
            {
                constexpr int f = 2 * (NU - 1);
                const u32 tbm2 = f ? T[f - 2] : NEG2, tbm1 = f ? T[f - 1] : topB;
                u32 vb;
                if constexpr (RU < R) {                        // row r0's interface of column j for the rows below (row skip)
                    static_assert(RU % 2 == 0 && RU >= 2, "r0 is even");
                    if_x0 = X[RU - 2]; if_x1 = X[RU - 1]; if_va = VbA;
                }
                if constexpr (f + 1 < RU) {
                    asm volatile(PC_B_PAIR
                                 : [vb] "=&v"(vb), [tb0] "+v"(T[f]), [tb1] "+v"(T[f + 1]), [ub0] "+v"(U[f]), [ub1] "+v"(U[f + 1])
                                 : [vpb] "v"(VbB), [tbm2] "v"(tbm2), [tbm1] "v"(tbm1), [tf] "v"(X[f]), [tg] "v"(X[f + 1]), [oe] "s"(OE2));
                } else {
                    asm volatile(PC_B_ODD
                                 : [vb] "=&v"(vb), [tb0] "+v"(T[f]), [ub0] "+v"(U[f])
                                 : [vpb] "v"(VbB), [tbm2] "v"(tbm2), [tbm1] "v"(tbm1), [tf] "v"(X[f]), [oe] "s"(OE2));
                }
                vbl = vb;
            }
            if constexpr (RU < R) if_vb = vbl;
            c2 = pk_sub(T[RU - 1], topB);
            top = topB;
#undef PC_M3
#undef PC_NOP
#undef PC_A1
#undef PC_A2
#undef PC_A3
#undef PC_A4
#undef PC_A5
#undef PC_A6
#undef PC_A7
#undef PC_A7I
#undef PC_A8
#undef PC_B1
#undef PC_B2
#undef PC_B3
#undef PC_B4
#undef PC_B5
#undef PC_B6
#undef PC_B7
#undef PC_B8
#undef PC_B9
#undef PC_B10
#undef PC_AB
#undef PC_AB_ODD
#undef PC_A_PAIR
#undef PC_A_ODD
#undef PC_B_PAIR
#undef PC_B_ODD
        };
#else
        // int16 lanes have no packed 3-input max: the cross-check kernel keeps six ops per cell pair and U = H~(rho, j-1).
        // Two columns at once, SKEWED: chain A walks column j, chain B column j+1 three rows behind,
        // on the same T/U registers (B reads what A has just produced and overwrites it in turn).
        // Each asm statement carries one row of A and one row of B interleaved instruction by
        // instruction, so every dependent pair of packed ops is separated by the other chain's op:
        // no s_nop, and the two chains give the VALU independent work (profiles/r01_ubench_row.txt:
        // 22.4 instead of 23.75 cycles per row at two waves per SIMD).  Only for blocks in which every
        // stream of the tile tracks the columns and none ends (the caller's fast path).
        auto column2 = [&](auto, const u32 (&S1)[K], const u32 (&S2)[K], u32 &c1, u32 &c2) {
            constexpr int L = 3, KP = 2;
            const u32 topA = pk_add(top, EPS2), topB = pk_add(topA, EPS2);     // T~(0,j), T~(0,j+1)
            u32 dhA[R], dhB[R];
            auto ind = [&](u32 (&dh)[R], const u32 (&S)[K], int q, u32 diag) {
                asm volatile(PC_MAX " %[uq], %[uq], %[tq]\n\t"
                             PC_ADD " %[dq], %[diag], %[s]"
                             : [dq] "=&v"(dh[q]), [uq] "+v"(U[q])
                             : [diag] "v"(diag), [s] "v"(S[COMBO[q]]), [tq] "v"(T[q]));
            };
#define PC_ONE_FULL                                                                    \
    PC_MAX " %[mn], %[dr], %[ur]\n\t"                                                  \
    PC_MAX " %[uq], %[uq], %[tq]\n\t"                                                  \
    PC_MAX " %[vs], %[vp], %[tu]\n\t"                                                  \
    PC_ADD " %[dq], %[dg], %[s]\n\t"                                                   \
    PC_MAX " %[mn], %[mn], %[vs]\n\t" "s_nop 0\n\t"                                    \
    PC_ADD " %[tn], %[mn], %[oe]"
#define PC_ONE_TAIL                                                                    \
    PC_MAX " %[mn], %[dr], %[ur]\n\t"                                                  \
    PC_MAX " %[vs], %[vp], %[tu]\n\t" "s_nop 0\n\t"                                    \
    PC_MAX " %[mn], %[mn], %[vs]\n\t" "s_nop 0\n\t"                                    \
    PC_ADD " %[tn], %[mn], %[oe]"
#define PC_PAIR_FULL                                                                   \
    PC_MAX " %[mna], %[dra], %[ura]\n\t"  PC_MAX " %[mnb], %[drb], %[urb]\n\t"         \
    PC_MAX " %[uqa], %[uqa], %[tqa]\n\t"  PC_MAX " %[uqb], %[uqb], %[tqb]\n\t"         \
    PC_MAX " %[vsa], %[vpa], %[tua]\n\t"  PC_MAX " %[vsb], %[vpb], %[tub]\n\t"         \
    PC_ADD " %[dqa], %[dga], %[sa]\n\t"   PC_ADD " %[dqb], %[dgb], %[sb]\n\t"          \
    PC_MAX " %[mna], %[mna], %[vsa]\n\t"  PC_MAX " %[mnb], %[mnb], %[vsb]\n\t"         \
    PC_ADD " %[tna], %[mna], %[oe]\n\t"   PC_ADD " %[tnb], %[mnb], %[oe]"
#define PC_PAIR_ATAIL                                                                  \
    PC_MAX " %[mna], %[dra], %[ura]\n\t"  PC_MAX " %[mnb], %[drb], %[urb]\n\t"         \
    PC_MAX " %[uqb], %[uqb], %[tqb]\n\t"                                               \
    PC_MAX " %[vsa], %[vpa], %[tua]\n\t"  PC_MAX " %[vsb], %[vpb], %[tub]\n\t"         \
    PC_ADD " %[dqb], %[dgb], %[sb]\n\t"                                                \
    PC_MAX " %[mna], %[mna], %[vsa]\n\t"  PC_MAX " %[mnb], %[mnb], %[vsb]\n\t"         \
    PC_ADD " %[tna], %[mna], %[oe]\n\t"   PC_ADD " %[tnb], %[mnb], %[oe]"
            // one row of one chain on its own (prologue of A, epilogue of B)
            auto row_alone = [&](u32 (&dh)[R], const u32 (&S)[K], int rr, u32 &Vprev, u32 &Tup) {
                u32 mn, vs;
                if (rr + KP < R) {
                    const int q = rr + KP;
                    asm volatile(PC_ONE_FULL
                                 : [mn] "=&v"(mn), [vs] "=&v"(vs), [uq] "+v"(U[q]), [tn] "=&v"(T[rr]), [dq] "=&v"(dh[q])
                                 : [vp] "v"(Vprev), [tu] "v"(Tup), [oe] "s"(OE2), [dg] "v"(T[q - 1]), [tq] "v"(T[q]),
                                   [s] "v"(S[COMBO[q]]), [dr] "v"(dh[rr]), [ur] "v"(U[rr]));
                } else {
                    asm volatile(PC_ONE_TAIL
                                 : [mn] "=&v"(mn), [vs] "=&v"(vs), [tn] "=&v"(T[rr])
                                 : [vp] "v"(Vprev), [tu] "v"(Tup), [oe] "s"(OE2), [dr] "v"(dh[rr]), [ur] "v"(U[rr]));
                }
                Tup = T[rr]; Vprev = vs;
            };
            // chain A alone for its first L rows
#pragma clang loop unroll(full)
            for (int q = 0; q < KP && q < R; ++q) ind(dhA, S1, q, q == 0 ? top : T[q - 1]);
            u32 TupA = topA, VpA = NEG2;
#pragma clang loop unroll(full)
            for (int r = 0; r < L && r < R; ++r) row_alone(dhA, S1, r, VpA, TupA);
            // chain B starts: its rows 0 and 1 read column j's T(0), T(1), which A has produced
#pragma clang loop unroll(full)
            for (int q = 0; q < KP && q < R; ++q) ind(dhB, S2, q, q == 0 ? topA : T[q - 1]);
            u32 TupB = topB, VpB = NEG2;
#pragma clang loop unroll(full)
            for (int r = L; r < R; ++r) {
                const int pb = r - L, qb = pb + KP;
                u32 mna, mnb, vsa, vsb;
                if (r + KP < R) {
                    const int qa = r + KP;
                    asm volatile(PC_PAIR_FULL
                                 : [mna] "=&v"(mna), [mnb] "=&v"(mnb), [vsa] "=&v"(vsa), [vsb] "=&v"(vsb),
                                   [uqa] "+v"(U[qa]), [uqb] "+v"(U[qb]), [tna] "=&v"(T[r]), [tnb] "=&v"(T[pb]),
                                   [dqa] "=&v"(dhA[qa]), [dqb] "=&v"(dhB[qb])
                                 : [vpa] "v"(VpA), [tua] "v"(TupA), [vpb] "v"(VpB), [tub] "v"(TupB), [oe] "s"(OE2),
                                   [dga] "v"(T[qa - 1]), [tqa] "v"(T[qa]), [sa] "v"(S1[COMBO[qa]]), [dra] "v"(dhA[r]), [ura] "v"(U[r]),
                                   [dgb] "v"(T[qb - 1]), [tqb] "v"(T[qb]), [sb] "v"(S2[COMBO[qb]]), [drb] "v"(dhB[pb]), [urb] "v"(U[pb]));
                } else {
                    asm volatile(PC_PAIR_ATAIL
                                 : [mna] "=&v"(mna), [mnb] "=&v"(mnb), [vsa] "=&v"(vsa), [vsb] "=&v"(vsb),
                                   [uqb] "+v"(U[qb]), [tna] "=&v"(T[r]), [tnb] "=&v"(T[pb]), [dqb] "=&v"(dhB[qb])
                                 : [vpa] "v"(VpA), [tua] "v"(TupA), [vpb] "v"(VpB), [tub] "v"(TupB), [oe] "s"(OE2),
                                   [dra] "v"(dhA[r]), [ura] "v"(U[r]),
                                   [dgb] "v"(T[qb - 1]), [tqb] "v"(T[qb]), [sb] "v"(S2[COMBO[qb]]), [drb] "v"(dhB[pb]), [urb] "v"(U[pb]));
                }
                TupA = T[r]; VpA = vsa; TupB = T[pb]; VpB = vsb;
            }
            c1 = pk_sub(T[R - 1], topA);               // column j's last row, before chain B overwrites it
#pragma clang loop unroll(full)
            for (int pb = (R > L ? R - L : 0); pb < R; ++pb) row_alone(dhB, S2, pb, VpB, TupB);
            c2 = pk_sub(T[R - 1], topB);
            top = topB;
#undef PC_ONE_FULL
#undef PC_ONE_TAIL
#undef PC_PAIR_FULL
#undef PC_PAIR_ATAIL
        };
#endif
#if PC_CHECK_RANGE
        auto note_range = [&]() {
#pragma clang loop unroll(full)
            for (int r = 0; r < R; ++r) { vmax = pk_max(vmax, pk_max(T[r], U[r])); vmin = pk_min(vmin, T[r]); }
        };
#endif
        uint4 q_lo = load_q(w_lo, n_lo, 0), q_hi = one_stream ? make_uint4(0u, 0u, 0u, 0u) : load_q(w_hi, n_hi, 0);
        u32 cur_lo = q_lo.x, cur_hi = q_hi.x;
        u32 nxt_lo = q_lo.y, nxt_hi = q_hi.y;
        u32 SA[K], SB[K], SC[K], SD[K];
        fetch_S(SA, cur_lo & 0xFF, cur_hi & 0xFF);
        // a new maximum somewhere in the NC columns from jb on (nb: the packed maximum over them and best2): resolve the
        // column, in visiting order (strict '>', the earlier column wins)
        auto take_maxima = [&](auto ncols, const u32 (&cs)[4], const u32 nb, const int jb) {
            constexpr int NC = decltype(ncols)::rows;
            if (nmax <= 65000) {
                u32 b = best2, ps = pos2;
#pragma clang loop unroll(full)
                for (int k = 0; k < NC; ++k) {
                    const u32 m = pk_maxq(b, cs[k]);
                    const u32 f = pk_minu(m ^ b, ONE2);              // 1 in the halves where column k is a new maximum
                    const u32 jk = (u32)(jb + k) * 0x00010001u;
                    ps = pk_madu(f, pk_subu(jk, ps), ps);            // their column becomes jb + k
                    b = m;
                }
                best2 = b; pos2 = ps; packed_ahead = true;
            } else {                                                  // columns beyond u16: the plain way
#pragma clang loop unroll(full)
                for (int k = 0; k < NC; ++k) {
                    const int cl = lo16(cs[k]) - PC_MLO * PC_EPS, ch = hi16(cs[k]) - PC_MHI * PC_EPS;
                    if (cl > bs_lo) { bs_lo = cl; bi_lo = a.m_lo; bj_lo = jb + k; }
                    if (ch > bs_hi) { bs_hi = ch; bi_hi = a.m_hi; bj_hi = jb + k; }
                }
                best2 = nb;
            }
        };
#if PC_SKIP
        // ---- row skip (the proposition and its proof: pc_bounds.h row_skip_plan).  A floored call owes exact records only to
        // pairs whose score reaches the floor F, and an alignment that does has M(r0, j) >= theta where it leaves register
        // row r0.  A stretch of fast-path blocks therefore runs column2 over the upper r0 rows alone, tests once per column
        // pair whether some stream has M(r0, .) >= theta, and computes the rows below only in the skip_w columns behind such
        // a column (and behind the stretch's first column: the one-column path before it computes every row and tests
        // nothing).  For the length of a stretch the rows below live in LDS (s_low: T~ and U per row and lane, U = H~(r, j - 1)
        // as on the one-column path), so that the column pair has their registers; while they are off they hold -infinity.
        // Whatever reads them as they stand after the stretch (the one-column path, the parked and the uniform last column)
        // reads lower bounds, which is all a cell below F needs.
        const int skip_w = a.skip_w > 0 ? a.skip_w : 0x3FFFFFFF;   // (a launch without a window: every row in every column)
        int low_until = 0;                                    // the rows below r0 are computed in the stretch's columns <= low_until
        bool low_on = false;                                  // ... and have been since they last held -infinity
        // (debug counters: 4-column blocks of the fast path, and those among them with the lower rows on -- both without the
        // blocks of a stretch's first window as long as nothing has triggered in it: they are on whatever the reads hold)
        u32 n_pair = 0, n_low = 0;
        int count_from = 0x7FFFFFFF;
        // the rows below r0 over the block's four columns, one pass over the rows: column k's diagonal term of the first of them
        // comes from dg[k] = T~(r0, j0 + k - 1), its V from vv[k] = V~(r0 + 1, j0 + k); the substitution terms are read from
        // the table again (this is the rare part: the column pairs' four sets need not stay in registers for it).
        // Top-aligned, the rows below the shorter adapter's last one are padding in its half: they are computed and stored
        // all the same, because the other half of the same packed registers is the longer adapter's real rows.
        auto lower_block = [&](u32 (&dg)[4], u32 (&vv)[4], u32 (&cs)[4]) {
            const char *srow[4];
#pragma clang loop unroll(full)
            for (int k = 0; k < 4; ++k) {
                const u32 bl = (cur_lo >> (8 * k)) & 0xFF;
#if PC_DUAL
                srow[k] = (const char *)s_tab + (u32)lut_one[bl];
#else
                const u32 bh = (cur_hi >> (8 * k)) & 0xFF;
                srow[k] = (const char *)s_tab + ((u32)lut_lo[bl] + (u32)lut_hi[one_stream ? bl : bh]);
#endif
            }
            u32 t[4] = {NEG2, NEG2, NEG2, NEG2};
#if PC_TOP
            u32 t_lo[4] = {NEG2, NEG2, NEG2, NEG2};                                   // T~(m_lo, .): the low half's own last row
            static_assert(PC_MLO > (PC_R0) && PC_MHI > (PC_R0) && (PC_MLO == PC_R || PC_MHI == PC_R), "both last rows lie below r0");
#endif
#pragma clang loop unroll(full)
            for (int r = PC_R0; r < R; ++r) {
                const uint2 tu = s_low[(r - PC_R0) * 64 + lane];
                u32 h = tu.y, tl = tu.x;                                              // H~(r, j0 - 1), T~(r, j0 - 1)
#pragma clang loop unroll(full)
                for (int k = 0; k < 4; ++k) {
                    h = pk_maxq(h, tl);                                               // H~(r, j0 + k)
                    const u32 sk = *(const u32 *)(srow[k] + 4 * COMBO[r]);
                    const u32 dnext = tl;                                             // T~(r, j0 + k - 1): the next row's diagonal
                    tl = pk_add(pk_maxq(pk_maxq(pk_add(dg[k], sk), h), vv[k]), OE2);  // T~(r, j0 + k)
                    vv[k] = pk_maxq(vv[k], tl);
                    dg[k] = dnext;
#if PC_TOP
                    if (r == PC_MLO - 1) t_lo[k] = tl;
                    if (r == PC_MHI - 1) t[k] = tl;
#else
                    t[k] = tl;
#endif
                }
                s_low[(r - PC_R0) * 64 + lane] = make_uint2(tl, h);                   // U = H~(r, j0 + 3): the one-column convention
            }
#if PC_TOP
#pragma clang loop unroll(full)
            for (int k = 0; k < 4; ++k) t[k] = (t_lo[k] & 0xFFFFu) | (t[k] & 0xFFFF0000u);   // the tracked term of each half: one packed select
#endif
            u32 tk = top;                                     // (top is T~(0, j0 + 3) now)
#pragma clang loop unroll(full)
            for (int k = 3; k >= 0; --k) { cs[k] = pk_sub(t[k], tk); tk = pk_sub(tk, EPS2); }
        };
#endif
        int jj = 0;                                           // columns since the last renormalisation
        bool u_ahead = false;                                 // wave-uniform, packed fp16 only: U[] already holds the coming column's H (column2)
        // the dword a block hands on at its end is the one two blocks ahead (0-based column j0 + 7); when
        // that opens a new 16-column block, the old one is used up -- its last dword is already in nxt -- and
        // the new one is requested at the block's head, a whole 4-column block of arithmetic before it is needed
        auto block_head = [&](const int j0) {
            const int kq = ((j0 + 7) >> 2) & 3;
            if (kq == 0) {
                q_lo = load_q(w_lo, n_lo, j0 + 7);
                if (!one_stream) q_hi = load_q(w_hi, n_hi, j0 + 7);
            }
            if (jj >= PC_KREN) {
                const u32 DK = pack2(PC_KREN * PC_EPS);
#pragma clang loop unroll(full)
                for (int r = 0; r < R; ++r) { T[r] = pk_sub(T[r], DK); U[r] = pk_sub(U[r], DK); }
                top = pk_sub(top, DK);
                jj = 0;
            }
        };
        auto block_tail = [&](const int j0) {
            const int kq = ((j0 + 7) >> 2) & 3;
            jj += 4;
            cur_lo = nxt_lo; cur_hi = nxt_hi;
            nxt_lo = pick_dw(q_lo, kq);
            if (!one_stream) nxt_hi = pick_dw(q_hi, kq);
        };
        for (int j0 = 1; j0 <= nmax; j0 += 4) {
            block_head(j0);
#if PC_SKIP
            if (j0 > tfmax && j0 + 3 < nmin) {
                // a stretch of fast-path blocks: the upper rows' U one column ahead, the rows below r0 into LDS -- with a window:
                // a path may have left row r0 in any column the one-column path ran
                if (packed_ahead) unpack_best();
                best2 = packbest(bs_lo, bs_hi);
                pos2 = ((u32)bj_lo & 0xFFFFu) | ((u32)bj_hi << 16);
#pragma clang loop unroll(full)
                for (int r = 0; r < PC_R0; ++r) U[r] = pk_maxq(U[r], T[r]);
#pragma clang loop unroll(full)
                for (int r = PC_R0; r < R; ++r) s_low[(r - PC_R0) * 64 + lane] = make_uint2(T[r], U[r]);
                low_until = j0 + 3 + skip_w; low_on = true;
                count_from = 0x7FFFFFFF;
                for (;;) {
                    // (three sets of substitution terms in flight, not four; row r0's interface of the first column pair
                    // stays in registers over the second)
                    fetch_S_up(SB, (cur_lo >> 8) & 0xFF, (cur_hi >> 8) & 0xFF);
                    fetch_S_up(SC, (cur_lo >> 16) & 0xFF, (cur_hi >> 16) & 0xFF);
                    const u32 tprev = T[PC_R0 - 1];           // T~(r0, j0 - 1)
                    u32 t0, t1, t2, t3;                       // M(r0, .) + r0 * eps of the four columns
                    column2(RowsT<PC_R0>{}, SA, SB, t0, t1);
                    const u32 p_x0 = if_x0, p_x1 = if_x1, p_va = if_va, p_vb = if_vb, p_m0 = T[PC_R0 - 2], p_m1 = T[PC_R0 - 1];
                    fetch_S_up(SD, cur_lo >> 24, cur_hi >> 24);
                    fetch_S_up(SA, nxt_lo & 0xFF, nxt_hi & 0xFF);
                    column2(RowsT<PC_R0>{}, SC, SD, t2, t3);
                    const u32 tr = pk_max(pk_max(pk_max(t0, t1), pk_max(t2, t3)), a.skip_thr2);
                    if (__any(tr != a.skip_thr2)) { low_until = j0 + 3 + skip_w; if (j0 < count_from) count_from = j0; }
                    if (j0 <= low_until) {
                        u32 dg[4] = {tprev, p_x1, p_m1, if_x1};
                        u32 vv[4] = {pk_maxq(pk_maxq(p_va, p_x0), p_x1), pk_maxq(pk_maxq(p_vb, p_m0), p_m1),
                                     pk_maxq(pk_maxq(if_va, if_x0), if_x1), pk_maxq(pk_maxq(if_vb, T[PC_R0 - 2]), T[PC_R0 - 1])};
                        u32 cs[4];
                        lower_block(dg, vv, cs);
                        low_on = true;
                        if (j0 >= count_from) ++n_low;
                        const u32 nb = pk_max(pk_max(best2, pk_max(cs[0], cs[1])), pk_max(cs[2], cs[3]));
                        if (__any(nb != best2)) take_maxima(RowsT<4>{}, cs, nb, j0);
                    } else if (low_on) {                      // the window has run out: nothing stale for a later one to read
#pragma clang loop unroll(full)
                        for (int r = PC_R0; r < R; ++r) s_low[(r - PC_R0) * 64 + lane] = make_uint2(NEG2, NEG2);
                        low_on = false;
                        if (j0 < count_from) count_from = j0;
                    }
                    block_tail(j0);
                    j0 += 4;
                    if (!(j0 + 3 < nmin)) break;
                    const int kq = ((j0 + 7) >> 2) & 3;
                    if (kq == 0) {
                        q_lo = load_q(w_lo, n_lo, j0 + 7);
                        if (!one_stream) q_hi = load_q(w_hi, n_hi, j0 + 7);
                    }
                    if (jj >= PC_KREN) {                          // the renormalisation, with the rows below r0 where they are
                        const u32 DK = pack2(PC_KREN * PC_EPS);
#pragma clang loop unroll(full)
                        for (int r = 0; r < PC_R0; ++r) { T[r] = pk_sub(T[r], DK); U[r] = pk_sub(U[r], DK); }
#pragma clang loop unroll(full)
                        for (int r = PC_R0; r < R; ++r) {
                            const uint2 tu = s_low[(r - PC_R0) * 64 + lane];
                            s_low[(r - PC_R0) * 64 + lane] = make_uint2(pk_sub(tu.x, DK), pk_sub(tu.y, DK));
                        }
                        top = pk_sub(top, DK);
                        jj = 0;
                    }
                }
                // the stretch is over: the rows below r0 back into their registers, as they stand (the upper rows' U needs no
                // conversion: the one-column path computes max(U, T), which is U)
#pragma clang loop unroll(full)
                for (int r = PC_R0; r < R; ++r) { const uint2 tu = s_low[(r - PC_R0) * 64 + lane]; T[r] = tu.x; U[r] = tu.y; }
                if (count_from < j0) n_pair += (u32)(j0 - count_from) / 4;
                if (j0 > nmax) break;
#if PC_KUP < PC_K
                fetch_S(SA, cur_lo & 0xFF, cur_hi & 0xFF);    // the one-column path reads the full row
#endif
                block_head(j0);
            }
            {
#else
            if (!PC_CHECK_RANGE && j0 > tfmax && j0 + 3 < nmin) {
                u32 c0, c1, c2, c3;
#if PC_F16
                if (!u_ahead) {                                   // entering from the one-column path: U = H~(rho, j0 - 1) -> H~(rho, j0)
#pragma clang loop unroll(full)
                    for (int r = 0; r < R; ++r) U[r] = pk_maxq(U[r], T[r]);
                    u_ahead = true;
                }
#endif
                fetch_S(SB, (cur_lo >> 8) & 0xFF, (cur_hi >> 8) & 0xFF);
                fetch_S(SC, (cur_lo >> 16) & 0xFF, (cur_hi >> 16) & 0xFF);
                fetch_S(SD, cur_lo >> 24, cur_hi >> 24);
                column2(RowsT<R>{}, SA, SB, c0, c1);
                fetch_S(SA, nxt_lo & 0xFF, nxt_hi & 0xFF);
                column2(RowsT<R>{}, SC, SD, c2, c3);
                const u32 nb = pk_max(pk_max(best2, pk_max(c0, c1)), pk_max(c2, c3));
                if (__any(nb != best2)) {
                    const u32 cs[4] = {c0, c1, c2, c3};
                    take_maxima(RowsT<4>{}, cs, nb, j0);
                }
            } else {
#endif
#if PC_CHECK_RANGE
#define PC_NOTE note_range();
#else
#define PC_NOTE
#endif
                if (packed_ahead) unpack_best();
                u_ahead = false;                                  // (nothing to convert: the column computes max(U, T), which is U)
                // (a tile whose streams all end in column nmax computes no column beyond it: T[] then IS the last column)
                const int last = uniform_fin ? nmax : 0x7FFFFFFF;
                fetch_S(SB, (cur_lo >> 8) & 0xFF, (cur_hi >> 8) & 0xFF);
                column(SlowT{}, j0, SA); PC_NOTE
                if (j0 + 1 <= last) {
                    fetch_S(SA, (cur_lo >> 16) & 0xFF, (cur_hi >> 16) & 0xFF);
                    column(SlowT{}, j0 + 1, SB); PC_NOTE
                    if (j0 + 2 <= last) {
                        fetch_S(SB, cur_lo >> 24, cur_hi >> 24);
                        column(SlowT{}, j0 + 2, SA); PC_NOTE
                        if (j0 + 3 <= last) {
                            fetch_S(SA, nxt_lo & 0xFF, nxt_hi & 0xFF);
                            column(SlowT{}, j0 + 3, SB); PC_NOTE
                        }
                    }
                }
                best2 = packbest(bs_lo, bs_hi);
                pos2 = ((u32)bj_lo & 0xFFFFu) | ((u32)bj_hi << 16);
            }
            block_tail(j0);
        }
        if (packed_ahead) unpack_best();
        // ---- the reads' last columns, all lanes at once: rolled re-run of the column from the parked
        // state, cells visited top to bottom with strict '>' (dp_scout.h:165-179).  The last column is the
        // last one the reference visits, so doing it after the loop keeps the visiting order.
        if (uniform_fin) {
            // T[r] = T~(r+1, n) of the tile's common last column n, top = T~(0, n): the candidates (rho, n), rho = 1..R, top to
            // bottom, strict '>' -- what the rolled re-run below derives from the parked state, read off the registers
#pragma clang loop unroll(full)
            for (int r = 0; r < R; ++r) {
                const u32 c = pk_sub(T[r], top);                     // M(rho, n) + rho*eps
#if PC_CHECK_RANGE
                PC_NOTE_V(c)
#endif
                const int il = r - pad_lo + 1, ih = r - pad_hi + 1;
                const int cl = lo16(c) - (r + 1) * PC_EPS, ch = hi16(c) - (r + 1) * PC_EPS;
                // (top-aligned: rows 1 .. m of each half, never a padding row below -- elsewhere r < R says nothing)
                if (have_lo && il >= 1 && r < PC_MLO && cl > bs_lo) { bs_lo = cl; bi_lo = il; bj_lo = n_lo; }
                if (have_hi && ih >= 1 && r < PC_MHI && ch > bs_hi) { bs_hi = ch; bi_hi = ih; bj_hi = n_hi; }
            }
        } else {
            const bool ev_lo = have_lo && tail_lo && n_lo > 0, ev_hi = have_hi && tail_hi && n_hi > 0;
            if (__any(ev_lo || ev_hi)) {
                const u32 topn = pk_add(ftop, EPS2);
                u32 diag = ftop, Tup = topn, Vprev = NEG2;
                const u32 *srow = (const u32 *)s_tab;
                const int bl = ev_lo ? w_lo[n_lo - 1] : 0;
                const int bh = one_stream ? bl : (ev_hi ? w_hi[n_hi - 1] : 0);
                const u32 rowbase = ((u32)lut_lo[bl] + (u32)lut_hi[bh]) / 4;
#pragma unroll 1
                for (int r = 0; r < R; ++r) {
                    const uint2 ol = ev_lo ? fin[r * 64 + lane] : make_uint2(0u, 0u);
#if PC_DUAL
                    const uint2 old = ol;
#else
                    const uint2 oh = ev_hi ? fin_hi_buf[r * 64 + lane] : make_uint2(0u, 0u);
                    const uint2 old = make_uint2((ol.x & 0xFFFFu) | (oh.x & 0xFFFF0000u), (ol.y & 0xFFFFu) | (oh.y & 0xFFFF0000u));
#endif
                    const u32 s = srow[rowbase + COMBO[r]];
                    const u32 d = pk_add(diag, s);
                    const u32 Hs = pk_max(old.y, old.x);
                    const u32 Vs = pk_max(Vprev, Tup);
                    const u32 Tn = pk_add(pk_max(pk_max(d, Hs), Vs), OE2);
                    diag = old.x; Tup = Tn; Vprev = Vs;
                    const u32 c = pk_sub(Tn, topn);                  // M(rho, n) + rho*eps, rho = r+1
#if PC_CHECK_RANGE
                    if (ev_lo || ev_hi) { PC_NOTE_V(d) PC_NOTE_V(Vs) PC_NOTE_V(Tn) PC_NOTE_V(c) PC_NOTE_V(pk_max(pk_max(d, Hs), Vs)) }
#endif
                    const int il = r - pad_lo + 1, ih = r - pad_hi + 1;
                    const int cl = lo16(c) - (r + 1) * PC_EPS, ch = hi16(c) - (r + 1) * PC_EPS;
                    if (ev_lo && il >= 1 && r < PC_MLO && cl > bs_lo) { bs_lo = cl; bi_lo = il; bj_lo = n_lo; }
                    if (ev_hi && ih >= 1 && r < PC_MHI && ch > bs_hi) { bs_hi = ch; bi_hi = ih; bj_hi = n_hi; }
                }
            }
        }
#if PC_SKIP
        if (a.skip_count && lane == 0 && n_pair) { atomicAdd(a.skip_count, (unsigned long long)n_pair); atomicAdd(a.skip_count + 1, (unsigned long long)n_low); }
#endif
#if PC_CHECK_RANGE
        {
            const int hi = lo16(vmax) > hi16(vmax) ? lo16(vmax) : hi16(vmax);
            const int lo = lo16(vmin) < hi16(vmin) ? lo16(vmin) : hi16(vmin);
            if (have_lo || have_hi) {
                atomicMax((int *)a.err + 4, hi); atomicMax((int *)a.err + 5, -lo);
                // the on-device assertion: outside what the lane type holds exactly -> the launch is reported as failed
                if (hi > (PC_F16 ? 2040 : 32000) || -lo > (PC_F16 ? 2040 : 32000)) atomicAdd(a.err, 1u);
            }
        }
#endif
        if (a.rec_out) {
            // (nchunks == 1: the end cell and its score are the whole answer -- what plan_kernel would make of the line below)
            if (have_lo) { int4 *o = (int4 *)(a.rec_out + p_lo * 8); o[0] = int4{-2, bj_lo + c0_lo, bi_lo, 0}; o[1] = int4{bs_lo, 0, 0, 0}; }
            if (have_hi) { int4 *o = (int4 *)(a.rec_out + p_hi * 8); o[0] = int4{-2, bj_hi + c0_hi, bi_hi, 0}; o[1] = int4{bs_hi, 0, 0, 0}; }
        } else {
            // (a chunk that starts beyond its window's end is never read by the planner -- it merges chunks 0 .. ceil(len / L) - 1 --
            // and is not written: a 4 Mb read among 20 kb reads makes two thousand chunks per window, ten of them real)
            const bool live_lo = have_lo && (chunk == 0 || n_lo > 0), live_hi = have_hi && (chunk == 0 || n_hi > 0);
            if (live_lo) { int4 o = {bs_lo, bi_lo, bj_lo + c0_lo, 0}; *(int4 *)(a.out + (p_lo * nchunks + chunk) * 4) = o; }
            if (live_hi) { int4 o = {bs_hi, bi_hi, bj_hi + c0_hi, 0}; *(int4 *)(a.out + (p_hi * nchunks + chunk) * 4) = o; }
        }
    }
}
)PCJIT";

}  // namespace pcj
