// pc_bounds.h -- score-scheme preconditions and the exact window bound of the two-pass scan.
//
// The reference allocates a full (|read|+1) x (|adapter|+1) trace matrix
// (seqan/align/dp_algorithm_impl.h:1547-1569).  For whole-read ("middle") scans this library
// instead (1) runs a score-only forward pass that finds the reference's max cell (I,J), then
// (2) recomputes with trace only columns [J - window, J].  That is exact, not heuristic:
//
//  * trace span W.  The traced path is an optimal path with score = best >= 0 (the cell
//    (m,0)=0 is always tracked).  Every gap character costs at least g = min(|open|,|ext|),
//    at most m diagonals earn at most `match` each, so #read-gap columns <= match*m/g and the
//    path touches at most  W = m + floor(match*m/g)  read columns left of J.
//
//  * warm-up span SPAN.  Column c of the window DP is started from a state every entry of
//    which is the score of a real path (row-0 free start followed by a vertical gap), so all
//    window values are <= the true ones, and equal as soon as the true optimum for that cell
//    is reached by a path starting inside the window.  Any path spanning s read columns
//    scores <= match*m - g*(s - m); every cell state has a trivial in-column alternative
//    scoring >= -(2|open| + (m-1)|ext|).  Hence paths with
//        s > m + (match*m + 2|open| + (m-1)|ext|)/g
//    are never optimal and all three states of every cell are exact from column
//    c + SPAN on,  SPAN = m + floor((match*m + 2|open| + (m-1)|ext|)/g) + 1.
//
//  * trace bits of column k depend on columns k-1 and k, so  window = W + SPAN + 1.
//
// Preconditions (checked, not assumed): match > 0, match > mismatch, open < 0, ext < 0, and every
// DP value must fit the packed int16 lanes the kernels compute in.  open == ext is the
// reference's linear-gap dispatch (seqan/align/global_alignment_unbanded.h:217-220), see below.
#pragma once
#include <stdint.h>

namespace pcb {

constexpr int MAX_ADAPTER = 128;     // rows the kernels can keep in registers
constexpr int NEG16 = -16384;        // "-infinity" of the int16 lanes; never wins a max

struct Bounds {
    int W;        // columns the traced path can span left of J
    int SPAN;     // warm-up columns before values are exact
    int window;   // W + SPAN + 1
};

// gap_open == gap_extend selects the reference's LINEAR-gap recurrence (one matrix; ties prefer
// diagonal, then vertical; no _correctTraceValue).  It is the affine recurrence with extension
// made impossible: with H_ext = V_ext = "-infinity" every gap cell is an "open" from M, the
// M-origin decisions (d >= max(H,V); V >= H) are exactly the linear ones, and the traceback takes
// one gap cell per step.  The kernels therefore run the same code with kLinearExtend.
constexpr int kLinearExtend = -12000;

inline bool is_linear(int gap_open, int gap_extend) { return gap_open == gap_extend; }

inline bool scores_supported(int match, int mismatch, int gap_open, int gap_extend, int max_m)
{
    if (!(match > 0 && match > mismatch && gap_open < 0 && gap_extend < 0)) return false;
    const long D = (long)match - mismatch;
    if (6 * D > 16000) return false;                         // spaced base codes 0..5*D in u16
    // linear mode adds -12000 to live values once per cell: keep them within +-4000
    const long lim = is_linear(gap_open, gap_extend) ? 4000 : 8000;
    if ((long)match * max_m > lim) return false;             // upper range of M
    if (2L * -gap_open + (long)max_m * -gap_extend > lim) return false;   // lower range of M,H,V
    if (-mismatch > lim || -gap_open > lim || -gap_extend > lim) return false;
    return true;
}

// Packed-FP16 traced kernel (pc_kernels.hip, trace16_kernel): every DP value X of register row
// rho (1..R), jj columns into the window, is held as the fp16 number  X + (rho + jj [+1]) * eps - C,
// eps = -gap_extend (drifting coordinates: gap extensions cost nothing).  fp16 represents every
// integer of magnitude <= 2048 exactly and adds them exactly, so the kernel is bit-exact as long as
// every value ever formed stays within +-kF16Limit.  True values: M <= match*R; the lowest finite
// value is a T = M + open of a lower-bound start state or a diagonal off it,
//   low = 3*open + (R-1)*ext + min(mismatch, 0)   (conservative),
// C puts `low` at -kF16Limit, and the window may then have at most max_cols columns before the
// drift reaches +kF16Limit.  ok = the scheme and R leave at least 32 columns.
constexpr int kF16Limit = 2040;
struct F16Plan { bool ok; int cen; int max_cols; };
inline F16Plan f16_plan(int match, int mismatch, int gap_open, int gap_extend, int R)
{
    F16Plan p = {false, 0, 0};
    if (is_linear(gap_open, gap_extend)) return p;           // linear mode replaces gap_extend by -12000
    if (!scores_supported(match, mismatch, gap_open, gap_extend, R)) return p;
    const long eps = -(long)gap_extend;
    const long low = 3L * gap_open + (long)(R - 1) * gap_extend + (mismatch < 0 ? mismatch : 0);
    const long high = (long)match * R;
    if (-mismatch > 1000 || -gap_open > 1000 || match > 1000 || eps > 500) return p;
    // the substitution terms sub - open + eps of the kernel's table must be exact fp16 integers too
    if (match - gap_open + eps > kF16Limit || mismatch - gap_open + eps > kF16Limit || mismatch - gap_open + eps < -kF16Limit) return p;
    // the tracked last-row term  T~(R,j) - top~(j) = M(R,j) + R*eps  is formed in fp16 as well (the scout's packed
    // compare): it must be an exact integer too.  (Found by tools/fuzz_parity.py: match 29, a 64-base adapter copied
    // exactly into a 150-column window -- 1856 + 448 = 2304 is not an fp16 integer, the score came out one off and
    // the walk's score check flagged the pair.)
    if (high + (long)R * eps > kF16Limit) return p;
    const long cols = (2L * kF16Limit - (high - low)) / eps - R - 2;
    if (cols < 32) return p;
    p.ok = true;
    p.cen = (int)(low + kF16Limit);
    p.max_cols = (int)(cols > (1 << 20) ? (1 << 20) : cols);
    return p;
}

// Run-time specialised score kernel (pc_jit_source.h): the same drifting coordinates, renormalised (shifted back
// down) every `kren` columns, values X held as X + (rho + jj [+1]) * eps - cen.  f16: the packed-fp16 variant
// (5 ops per cell pair) is usable -- every value formed, the tracked term M + R*eps included, an exact fp16
// integer -- otherwise packed int16 (6 ops); ok = false: the scheme leaves no useful period (generic kernels).
struct SpecPlan { bool ok, f16; long kren, cen; };
inline SpecPlan spec_plan(int match, int mismatch, int gap_open, int gap_extend, int R, bool force_int16)
{
    SpecPlan p = {false, false, 0, 0};
    const long eps = -(long)gap_extend;
    const long low = 2L * gap_open + (long)(R - 1) * gap_extend < (long)gap_open + (long)(R - 1) * gap_extend + mismatch
                         ? 2L * gap_open + (long)(R - 1) * gap_extend
                         : (long)gap_open + (long)(R - 1) * gap_extend + mismatch;
    const long low2 = low < (long)gap_open ? low : (long)gap_open;
    const long high = (long)match * R;
    auto period = [&](long lim) -> long {
        const long k = (2 * lim - (high - low2) - (long)(R + 6) * eps) / eps;
        return k < 0 ? 0 : (k / 4 * 4 < (1L << 20) ? k / 4 * 4 : (1L << 20));
    };
    p.f16 = !force_int16 && period(kF16Limit) >= 64 && high + (long)R * eps <= kF16Limit && -mismatch <= 1000 && -gap_open <= 1000;
    const long lim = p.f16 ? kF16Limit : 32000;
    p.kren = period(lim);
    p.ok = p.kren >= 64;
    p.cen = low2 + lim;
    return p;
}

// ---- Row skip of the specialised score kernel's fast path (pc_jit_source.h, PC_SKIP) ----------------------------------
//
// A floored two-pass call (pc_scan_device_floored) answers a pair whose best score is below its floor F with "no
// alignment"; its score record is never shown.  Pass 1 therefore owes exact end cells only to pairs that reach F.
//
// Setting.  R register rows 1..R, the shorter adapter of a pair bottom-aligned under `pad` rows that keep M = 0 like
// row 0.  The scheme has match > 0, mismatch <= match, gap_open < 0, gap_extend < 0 (anything else is refused; g =
// min(|gap_open|, |gap_extend|) is the least any gap character costs).  r0 is an even register row, pad < r0 < R.  Per
// half, with m its real rows and F its floor,
//     theta = F - match * (R - r0)                               and it must be > 0 (refused otherwise),
//     W_low = (R - r0) + max over the halves of floor(max(0, match * m - F) / g).
// The variant computes rows <= r0 in every column, and rows > r0 only in the columns j'' .. j'' + W_low behind a column
// j'' with M(r0, j'') >= theta in either half (more columns do no harm: see 1); where it switches them on, their values
// of the column before are -infinity or whatever an earlier window left.  Call what it computes M^.
//
//  1. M^ <= M everywhere.  Rows <= r0 never read a row below them, so they are exact.  Below r0 every value is a maximum
//     over a SUBSET of the paths the full recurrence maximises over (each computed cell is fed true row-r0 values and
//     values of computed cells or -infinity), and each of those paths is a real one.
//  2. Every candidate end cell c -- last row, or last column at any row -- with M(c) >= F has M^(c) = M(c).  If c lies in
//     a row <= r0 there is nothing to show.  Otherwise take an optimal path to c.  It starts with score 0 in row 0 (or a
//     padding row, which is the same thing) or in column 0.
//       (a) It starts in column 0 in a row > r0: then it has at most R - r0 - 1 diagonals and scores at most
//           match * (R - r0 - 1) < match * (R - r0) < F because theta > 0.  Contradiction.  (This is the host's "column-0
//           condition": theta > 0 for every half.)
//       (b) So it has cells in row r0; let (r0, j'') be the last one.  The prefix up to it, in whatever state it is there
//           (a vertical gap running through row r0 included: V <= M), scores <= M(r0, j'').  The rest passes at most
//           R - r0 rows, earns at most `match` per row and nothing from gaps, so M(r0, j'') >= F - match * (R - r0) =
//           theta: column j'' switches the lower rows on.
//       (c) The path goes on to (r0 + 1, j'') -- vertically -- or to (r0 + 1, j'' + 1) -- diagonally.  Both are fed from
//           row r0's values of columns j'' - 1 and j'' (T of the diagonal neighbour, V and T of the upper one), which are
//           exact, and lie in columns that are switched on.
//       (d) Behind column j'' the path has at most R - r0 diagonal steps, and h horizontal gap characters with
//           match * m - g * h >= F, so it ends at a column <= j'' + (R - r0) + floor((match * m - F) / g) <= j'' + W_low:
//           every cell of it below row r0 lies in a computed column, and by induction along the path M^ of each such
//           cell is at least the path's score there.  With 1, M^(c) = M(c).
//  3. Consequences.  max over the candidates of M^ equals that of M whenever the latter is >= F, and then the sets of cells
//     attaining it agree, so strict '>' in visiting order picks the same end cell: the records of pairs >= F are bit-identical.
//     A pair below F stays below F (1), is counted by pc_floor_skipped and answered by plan_kernel exactly as before.
//  Chunked launches: a cell >= F has its whole path inside W <= SPAN columns, so the lead-in argument above stands; a chunk's
//  first tracked column is reached through the one-column path, which computes every row, and entering the fast path from
//  it switches the lower rows on for W_low columns (a path may have left row r0 in any column the one-column path ran).
//
// The rule for r0 (row_skip_r0) is a function of the kernel's recipe alone -- r0 is a compile-time constant of the ONE
// kernel per adapter pair -- and has no part in exactness: the smallest even row above the padding for which the share
// of column pairs with the lower rows on stays under 1 / 64 in a model of uniform random bases at the floor of a 90 %
// identity threshold (--middle_threshold's default, Pipeline.identity_score_bound), F = floor(m * (0.9 * match - 0.1 *
// max(|mismatch|, |gap_open|, |gap_extend|))): per half the chance
// that an ungapped m'-row prefix (m' = the half's real rows down to r0) loses at most match * m' - theta, times 128 cells per
// column pair and half, times the W_low / 2 + 1 column pairs a window lasts.  R (no skipping path in the kernel) if no
// row at least four above the last one qualifies.  The model leaves gapped prefixes out, which are some ten times as
// frequent, and a lower threshold triggers more often: either costs time, never exactness.  Measured on the headline
// (profiles/score_row_skip_before_after.txt): the rule's row, 20 for both pairs, is the fastest of 14 .. 24.
// At most kRowSkipMaxLower rows are left below r0: the variant keeps them in LDS, 512 bytes per row and workgroup, and
// twelve one-wave workgroups (three waves per SIMD) share a CU's 160 KiB, so that 16 rows (8 KiB) beside the kernel's
// tables (at most 100 * K + 1536 bytes, K <= 28 in that register class) leave the occupancy to the registers, as it was.
// pc_jit.cpp gives the variant to three-wave kernels only and checks these bytes again.
constexpr int kRowSkipMaxLower = 16;
struct RowSkip { bool ok; int theta_lo, theta_hi, w_low; };
inline bool row_skip_scheme(int match, int mismatch, int gap_open, int gap_extend)
{
    return match > 0 && mismatch <= match && gap_open < 0 && gap_extend < 0 && !is_linear(gap_open, gap_extend);
}
// thresholds and window for one launch: F_lo / F_hi are the halves' floors (the lowest floor of any job the launch serves)
inline RowSkip row_skip_plan(int match, int mismatch, int gap_open, int gap_extend, int R, int r0, int m_lo, int m_hi,
                             long F_lo, long F_hi)
{
    RowSkip p = {false, 0, 0, 0};
    if (!row_skip_scheme(match, mismatch, gap_open, gap_extend)) return p;
    if (m_lo < 1 || m_hi < 1 || m_lo > R || m_hi > R || (m_lo != R && m_hi != R)) return p;
    const int pad = R - (m_lo < m_hi ? m_lo : m_hi);
    if (r0 < 2 || (r0 & 1) || r0 >= R || r0 <= pad) return p;
    const long below = (long)match * (R - r0);
    const long t_lo = F_lo - below, t_hi = F_hi - below;
    if (t_lo <= 0 || t_hi <= 0) return p;                                    // 2 (a): the column-0 condition
    // a floor nothing can reach never triggers; one beyond what the lane type adds exactly must not reach the kernel
    if (F_lo > (long)match * m_lo || F_hi > (long)match * m_hi) return p;
    const long g = -gap_open < -gap_extend ? -(long)gap_open : -(long)gap_extend;
    const long h_lo = ((long)match * m_lo - F_lo) / g, h_hi = ((long)match * m_hi - F_hi) / g;
    const long w = (R - r0) + (h_lo > h_hi ? h_lo : h_hi);
    if (w > (1L << 20)) return p;
    p.ok = true; p.theta_lo = (int)t_lo; p.theta_hi = (int)t_hi; p.w_low = (int)w;
    return p;
}
inline long row_skip_nominal_floor(int match, int mismatch, int gap_open, int gap_extend, int m)
{
    long P = -mismatch > -gap_open ? -(long)mismatch : -(long)gap_open;
    if (-(long)gap_extend > P) P = -(long)gap_extend;
    const long f = ((long)m * (9L * match - P)) / 10;                 // floor: the product is >= 0 where it is used
    return f;
}
inline int row_skip_r0(int match, int mismatch, int gap_open, int gap_extend, int R, int m_lo, int m_hi)
{
    if (!row_skip_scheme(match, mismatch, gap_open, gap_extend) || match == mismatch) return R;
    const long F_lo = row_skip_nominal_floor(match, mismatch, gap_open, gap_extend, m_lo);
    const long F_hi = row_skip_nominal_floor(match, mismatch, gap_open, gap_extend, m_hi);
    if (F_lo <= 0 || F_hi <= 0) return R;
    const int first = R - kRowSkipMaxLower > 2 ? (R - kRowSkipMaxLower + 1) / 2 * 2 : 2;   // even, and R - first <= kRowSkipMaxLower
    for (int r0 = first; r0 <= R - 4; r0 += 2) {
        const RowSkip p = row_skip_plan(match, mismatch, gap_open, gap_extend, R, r0, m_lo, m_hi, F_lo, F_hi);
        if (!p.ok) continue;
        double rate = 0;
        for (int half = 0; half < 2; ++half) {
            const int mp = (half ? m_hi : m_lo) - (R - r0);                  // real rows down to r0
            const long theta = half ? p.theta_hi : p.theta_lo;
            const long kmax = ((long)match * mp - theta) / ((long)match - mismatch);   // mismatches an ungapped prefix can afford
            if (kmax < 0) continue;
            double term = 1.0, sum = 0;                                      // C(mp, k) * 0.75^k * 0.25^(mp - k), from k = 0
            for (int i = 0; i < mp; ++i) term *= 0.25;
            for (long k = 0; k <= kmax && k <= mp; ++k) { sum += term; term *= 3.0 * (double)(mp - k) / (double)(k + 1); }
            rate += 128.0 * sum;
        }
        if (rate * (p.w_low / 2 + 1) <= 1.0 / 64) return r0;
    }
    return R;
}

// ---- The same row skip with the shorter adapter TOP-aligned (pc_jit_source.h, PC_TOP) ---------------------------------
//
// Setting.  Register row rho = adapter row rho in BOTH halves: a half of m rows fills register rows 1..m, and the rows
// m + 1..R of the shorter half are padding BELOW it (a letter that scores 0 against everything).  Nothing a real row
// computes reads a row below it, so the real rows are what they would be without the padding; a padding row is never a
// candidate end cell and nothing reads it (its values are maxima and sums of real ones and of 0: inside the same range).
// r0 is an even register row with 2 <= r0 < min(m_lo, m_hi): the last row of BOTH halves lies below r0, so neither half's
// end cells have to be tracked by the part that runs in every column.  Per half, with m its rows and F its floor,
//     theta = F - match * (m - r0)                               and it must be > 0 (refused otherwise),
//     W_low = max over the halves of (m - r0) + floor(max(0, match * m - F) / g).
// The variant computes rows <= r0 in every column and rows > r0 only in the columns j'' .. j'' + W_low behind a column
// j'' with M(r0, j'') >= theta in either half.  Call what it computes M^.
//
//  1. M^ <= M everywhere, and rows <= r0 are exact: as above, word for word.
//  2. Every candidate end cell c of a half -- row m at any column, or the last column at a row 1..m -- with M(c) >= F has
//     M^(c) = M(c).  If c lies in a row <= r0 there is nothing to show.  Otherwise take an optimal path to c; it lies in
//     rows <= m (paths only ever go down), starts with score 0 in row 0 or in column 0.
//       (a) It starts in column 0 in a row > r0: then it has at most m - r0 - 1 diagonals and scores at most
//           match * (m - r0 - 1) < match * (m - r0) < F because theta > 0.  Contradiction.
//       (b) So it has cells in row r0; let (r0, j'') be the last one.  The prefix up to it scores <= M(r0, j''); the rest
//           passes at most m - r0 rows, earns at most `match` per row and nothing from gaps, so M(r0, j'') >= F - match *
//           (m - r0) = theta: column j'' switches the lower rows on.
//       (c) The step off row r0 is fed from row r0's exact values of columns j'' - 1 and j'', in columns that are on.
//       (d) Behind column j'' the path has at most m - r0 diagonal steps and h horizontal gap characters with match * m -
//           g * h >= F, so it ends at a column <= j'' + (m - r0) + floor((match * m - F) / g) <= j'' + W_low.  By
//           induction along the path M^ of each of its cells is at least the path's score there; with 1, M^(c) = M(c).
//  3. The consequences, and the chunked launches' lead-in, are those of the bottom-aligned layout.
// What the layout buys: no padding sits above r0, so all r0 always-on rows are real in both halves, and theta of the
// short half is F - match * (m_short - r0) instead of F - match * (R - r0) -- out of random sequence's reach in r0 real
// rows -- so r0 can sit lower at the same share of columns with the lower rows on.
// For m_lo == m_hi == R the two layouts are one: the plans agree in every field.
inline RowSkip row_skip_plan_top(int match, int mismatch, int gap_open, int gap_extend, int R, int r0, int m_lo, int m_hi,
                                 long F_lo, long F_hi)
{
    RowSkip p = {false, 0, 0, 0};
    if (!row_skip_scheme(match, mismatch, gap_open, gap_extend)) return p;
    if (m_lo < 1 || m_hi < 1 || m_lo > R || m_hi > R || (m_lo != R && m_hi != R)) return p;
    const int m_min = m_lo < m_hi ? m_lo : m_hi;
    if (r0 < 2 || (r0 & 1) || r0 >= m_min) return p;                         // both last rows below r0
    const long t_lo = F_lo - (long)match * (m_lo - r0), t_hi = F_hi - (long)match * (m_hi - r0);
    if (t_lo <= 0 || t_hi <= 0) return p;                                    // 2 (a): the column-0 condition
    if (F_lo > (long)match * m_lo || F_hi > (long)match * m_hi) return p;
    const long g = -gap_open < -gap_extend ? -(long)gap_open : -(long)gap_extend;
    const long w_lo = (m_lo - r0) + ((long)match * m_lo - F_lo) / g, w_hi = (m_hi - r0) + ((long)match * m_hi - F_hi) / g;
    const long w = w_lo > w_hi ? w_lo : w_hi;
    if (w > (1L << 20)) return p;
    p.ok = true; p.theta_lo = (int)t_lo; p.theta_hi = (int)t_hi; p.w_low = (int)w;
    return p;
}

// The rule for r0 in the top-aligned layout.  The closed form of row_skip_r0 counts ungapped prefixes only; with the
// short half's threshold out of random sequence's reach the long half decides, and there gapped prefixes are some 260
// times as frequent as ungapped ones at the rows in question (simulated): the closed form answers 14 for the 28 | 22
// pair, a row at which the lower rows would be on most of the time.  So the rate is MEASURED instead: the plain affine
// recurrence of each half's first rows (sets_lo / sets_hi: the rows' 5-bit sets over the read codes, pc_letters.h) over
// kRowSkipSimColumns columns of seeded uniform random bases, counting per candidate row the columns with M(r0, j) >=
// theta at the nominal floors of a 90 % threshold.  A wave holds 64 lanes and a block is 4 columns: the share of blocks
// with the lower rows on is modelled as  events per column * 256 * (W_low / 4 + 1),  and the rule takes the smallest even
// row, at least four above the last register row and with at most kRowSkipMaxLower rows below it, whose share stays under
// 1 / 32.  A function of the recipe alone (the seed is fixed), and no part of exactness: a bad row costs time only.
// Measured on the headline (profiles/score_top_layout_before_after.txt).
constexpr long kRowSkipSimColumns = 1L << 20;
inline int row_skip_r0_top(int match, int mismatch, int gap_open, int gap_extend, int R, int m_lo, int m_hi,
                           const unsigned char *sets_lo, const unsigned char *sets_hi)
{
    if (!row_skip_scheme(match, mismatch, gap_open, gap_extend) || match == mismatch) return R;
    if (m_lo < 1 || m_hi < 1 || m_lo > R || m_hi > R || R > MAX_ADAPTER) return R;
    const long F[2] = {row_skip_nominal_floor(match, mismatch, gap_open, gap_extend, m_lo),
                       row_skip_nominal_floor(match, mismatch, gap_open, gap_extend, m_hi)};
    if (F[0] <= 0 || F[1] <= 0) return R;
    const int m_min = m_lo < m_hi ? m_lo : m_hi;
    const int first = R - kRowSkipMaxLower > 2 ? (R - kRowSkipMaxLower + 1) / 2 * 2 : 2;
    int last = (m_min - 1) / 2 * 2;                                          // even, < m_min
    if (last > R - 4) last = (R - 4) / 2 * 2;
    if (last < first) return R;
    long events[MAX_ADAPTER + 1] = {0};
    bool usable[MAX_ADAPTER + 1] = {false};
    RowSkip plan[MAX_ADAPTER + 1];
    bool any = false;
    for (int r0 = first; r0 <= last; r0 += 2) {
        plan[r0] = row_skip_plan_top(match, mismatch, gap_open, gap_extend, R, r0, m_lo, m_hi, F[0], F[1]);
        usable[r0] = plan[r0].ok; any = any || plan[r0].ok;
    }
    if (!any) return R;
    for (int h = 0; h < 2; ++h) {
        const unsigned char *sets = h ? sets_hi : sets_lo;
        long theta[MAX_ADAPTER + 1];
        for (int r0 = first; r0 <= last; r0 += 2) theta[r0] = usable[r0] ? (h ? plan[r0].theta_hi : plan[r0].theta_lo) : (1L << 40);
        int M[MAX_ADAPTER + 1], H[MAX_ADAPTER + 1];
        for (int i = 0; i <= last; ++i) { M[i] = 0; H[i] = -(1 << 28); }
        uint64_t x = 0x9E3779B97F4A7C15ull;                                  // xorshift64*, 32 bases per draw; both halves read the same columns
        uint64_t bits = 0; int have = 0;
        for (long j = 0; j < kRowSkipSimColumns; ++j) {
            if (!have) { x ^= x >> 12; x ^= x << 25; x ^= x >> 27; bits = x * 0x2545F4914F6CDD1Dull; have = 32; }
            const int code = (int)(bits & 3); bits >>= 2; --have;
            int diag = 0, upM = 0, upV = -(1 << 28);
            for (int i = 1; i <= last; ++i) {
                const int hh = H[i] + gap_extend > M[i] + gap_open ? H[i] + gap_extend : M[i] + gap_open;
                const int vv = upV + gap_extend > upM + gap_open ? upV + gap_extend : upM + gap_open;
                int best = diag + (((sets[i - 1] >> code) & 1) ? match : mismatch);
                if (hh > best) best = hh;
                if (vv > best) best = vv;
                diag = M[i]; M[i] = best; H[i] = hh; upM = best; upV = vv;
            }
            for (int r0 = first; r0 <= last; r0 += 2) events[r0] += M[r0] >= theta[r0];
        }
    }
    for (int r0 = first; r0 <= last; r0 += 2) {
        if (!usable[r0]) continue;
        const double share = (double)events[r0] / (double)kRowSkipSimColumns * 256.0 * (plan[r0].w_low / 4 + 1);
        if (share <= 1.0 / 32) return r0;
    }
    return R;
}

// PC_JIT_R0 (measurements): the row the environment asks for in place of row_skip_r0's, for the pair of adapters of m_a and m_b
// bases.  "20": that row for every pair.  "28|22:20,33|30:22": a row per pair, named by both of its lengths in either order; a
// pair that is not listed keeps rule_r0.  Anything else -- an empty entry, a missing part, a stray character -- sets *malformed
// and the whole text is ignored (rule_r0): a typo must not pass for a measurement.  The caller still checks that the row is usable.
inline int row_skip_r0_override(const char *spec, int m_a, int m_b, int rule_r0, bool *malformed)
{
    *malformed = false;
    auto number = [](const char *&q, int &v) {
        if (*q < '0' || *q > '9') return false;
        v = 0;
        while (*q >= '0' && *q <= '9' && v < 100000) v = v * 10 + (*q++ - '0');
        return true;
    };
    const char *q = spec;
    int first = 0;
    if (!q || !number(q, first)) { *malformed = true; return rule_r0; }
    if (!*q) return first;                                   // one row for every pair
    int found = rule_r0;
    q = spec;
    for (;;) {
        int a = 0, b = 0, row = 0;
        if (!number(q, a) || *q++ != '|' || !number(q, b) || *q++ != ':' || !number(q, row)) { *malformed = true; return rule_r0; }
        if ((a == m_a && b == m_b) || (a == m_b && b == m_a)) found = row;
        if (!*q) return found;
        if (*q++ != ',') { *malformed = true; return rule_r0; }
    }
}

inline bool compute_bounds(int match, int mismatch, int gap_open, int gap_extend, int m, Bounds &b)
{
    if (!scores_supported(match, mismatch, gap_open, gap_extend, m > 0 ? m : 1)) return false;
    const int go = -gap_open, ge = -gap_extend;
    const int g = go < ge ? go : ge;
    b.W = m + (match * m) / g;
    b.SPAN = m + (match * m + 2 * go + (m - 1) * ge) / g + 1;
    b.window = b.W + b.SPAN + 1;
    return true;
}

}  // namespace pcb
