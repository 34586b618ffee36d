// pc_middle_paths.h -- the path of a MIDDLE hit from a bounded window of the masked read.  pcpath::align_path
// (pc_paths.h) restated with four differences; written once for device (pc_middle_paths.hip: one lane per hit) and host
// (tests/host/test_middle_paths.cpp compares every result with align_path over the whole, explicitly masked read).
//
// A middle hit is the alignment of an adapter against the whole trimmed read of n bases, with the read intervals of the
// read's earlier hits replaced by '-' (Dna5 code 4).  Masking is in place, so coordinates never move, and the hit list
// alone rebuilds the read a hit was aligned against.  What the list also gives is the hit's exclusive read end `re`.
//
//   window      the DP runs over global columns c0 + 1 .. c1,  c1 = min(n, re + W),  c0 = max(0, re - window), with W and
//               window of pcb::compute_bounds for the adapter's own length (hit_window()).  A scheme compute_bounds
//               refuses gets the whole read: c0 = 0, c1 = n.
//   start state c0 == 0: align_path's (M(i) = 0, H(i) = -inf).  c0 > 0: the lower-bound state of pc_bounds.h, a row-0
//               start followed by a vertical gap: M(i) = gap_open + (i - 1) * gap_extend, H(i) = -inf (with
//               gap_open == gap_extend that is the linear dispatch's i * gap).
//   scout       the same visiting order and strict '>', from (0 at (m, c0)).  The cells of the window's last column are
//               candidates only when that column is the read's last (c1 == n); last-row cells always are.  The end cell
//               is not forced.
//   mask        is the caller's rd(k): code 4 for every GLOBAL k inside one of the hit's earlier intervals.
// The walk is pcw::Walk with col0 = c0 and n_total = n: the record and head[1] (= c0 + its local column) are in
// trimmed-read coordinates, local columns 1 .. c1 - c0 index the trace, and "left the window" stays an error.
//
// Why this is exact:
//   * every window value is the score of a real path, hence <= the true value, hence <= the hit's score S*; S* > 0
//     because a hit has a match;
//   * the true end cell J* satisfies re <= J* <= re + (W - m): it differs from re only by a trailing read-gap run;
//   * all three states of a cell are exact from column c0 + SPAN on, and J* - c0 >= window = W + SPAN + 1, so every cell
//     the path touches, and the column before it, is exact;
//   * a candidate earlier in visiting order with window value S* would have true value S* and would have been the
//     reference's choice.  So the scout lands on the same cell with the same H / V tie, and the trace bits along the
//     path are the reference's.
#pragma once
#include "pc_paths.h"

namespace pcpath {

// bounded: compute_bounds accepted the scheme for this adapter length (W, window are its)
PC_HD void hit_window(int n, int re, bool bounded, int W, int window, int &c0, int &c1)
{
    c0 = 0; c1 = n;
    if (!bounded) return;
    const long long hi = (long long)re + W, lo = (long long)re - window;
    c1 = hi < n ? (int)hi : n;
    c0 = lo > 0 ? (int)lo : 0;
    if (c0 > c1) c0 = c1;
}

// Mem, ad, sink: as align_path, the trace indexed by LOCAL columns j = 1 .. c1 - c0.
// rd(k): Dna5 code of the k-th (0-based, GLOBAL) base of the masked read; only k in [c0, c1) is asked for.
// -> 0, or 1 if the walk reported an inconsistency (leaving the window included) or did not end within its step bound.
// n or m == 0, or an empty window: the reference's failure record, a zero head, no operations.
template <typename Mem, typename RdFn, typename AdFn, typename Sink>
PC_HD int align_path_window(int n, int m, int c0, int c1, RdFn rd, AdFn ad, int match, int mismatch, int gap_open,
                            int gap_extend, Mem mem, pcw::Digest &out, int32_t head[4], Sink sink)
{
    head[0] = 0; head[1] = 0; head[2] = 0; head[3] = 0;
    const int nc = c1 - c0;
    if (n <= 0 || m <= 0 || nc <= 0) {
        out.read_start = -1; out.read_end = 0; out.adapter_start = -1; out.adapter_end = 0; out.score = INT_MIN;
        out.matches = 0; out.aligned_len = 0; out.full_len = 0;
        return 0;
    }
    const bool linear = gap_open == gap_extend;
    if (c0 == 0) for (int i = 1; i <= m; ++i) { mem.M(i) = 0; mem.H(i) = NEG_INF; }
    else for (int i = 1; i <= m; ++i) { mem.M(i) = gap_open + (i - 1) * gap_extend; mem.H(i) = NEG_INF; }
    const bool last_is_reads = c1 == n;
    int bestM = 0, bestH = NEG_INF, bestV = NEG_INF, bestI = m, bestJ = 0;
    for (int j = 1; j <= nc; ++j) {
        int diag = 0, upM = 0, upV = NEG_INF;          // row 0: M = 0, V = -inf
        const int h = rd(c0 + j - 1);
        const bool last_col = last_is_reads && j == nc;
        uint32_t word = 0;
        for (int i = 1; i <= m; ++i) {
            const int Mi = mem.M(i);
            const int sub = (h == ad(i - 1)) ? match : mismatch;
            int S, Hs = NEG_INF, Vs = NEG_INF, nib;
            if (linear) {
                S = diag + sub; nib = pcw::NIB_HOPEN | pcw::NIB_VOPEN;
                int t = upM + gap_extend;
                if (S < t) { S = t; nib |= pcw::NIB_NOTDIAG; }
                t = Mi + gap_extend;
                if (S < t) { S = t; nib |= pcw::NIB_NOTDIAG | pcw::NIB_FROMH; }
            } else {
                nib = 0;
                Hs = mem.H(i) + gap_extend;
                int t = Mi + gap_open;
                if (Hs < t) { Hs = t; nib |= pcw::NIB_HOPEN; }
                Vs = upV + gap_extend;
                t = upM + gap_open;
                if (Vs < t) { Vs = t; nib |= pcw::NIB_VOPEN; }
                S = Vs;
                if (S < Hs) { S = Hs; nib |= pcw::NIB_FROMH; }
                const int d = diag + sub;
                if (S <= d) S = d; else nib |= pcw::NIB_NOTDIAG;
                mem.H(i) = Hs;
            }
            diag = Mi;
            mem.M(i) = S;
            upM = S; upV = Vs;
            const int slot = (i - 1) & (ROWS_PER_WORD - 1);
            word |= (uint32_t)nib << (4 * slot);
            if (slot == ROWS_PER_WORD - 1 || i == m) { mem.put(j, (i - 1) / ROWS_PER_WORD, word); word = 0; }
            if ((last_col || i == m) && S > bestM) { bestM = S; bestH = Hs; bestV = Vs; bestI = i; bestJ = j; }
        }
    }
    int tie_fix = 0;
    if (!linear) tie_fix = (bestV == bestM) ? 1 : (bestH == bestM) ? 2 : 0;
    pcw::Walk w;
    w.start(bestI, bestJ, m, c0, n, bestM, tie_fix);
    const int cap = nc + m + 8;                        // a path inside the window has at most nc + m steps
    int overrun = 0, k = 0;
    uint32_t acc = 0;
    while (!w.done) {
        if (k >= cap) { overrun = 1; break; }
        const int c = w.col, r = w.row;
        const int nib = (int)(mem.get(c, (r - 1) / ROWS_PER_WORD) >> (4 * ((r - 1) & (ROWS_PER_WORD - 1)))) & 15;
        const bool eq = rd(c0 + c - 1) == ad(r - 1);
        w.consume(nib, eq);
        const bool dcol = w.col != c, drow = w.row != r;
        const uint32_t op = (dcol && drow) ? (eq ? OP_EQ : OP_X) : (drow ? OP_D : OP_I);
        acc |= op << (2 * (k & (OPS_PER_WORD - 1)));
        ++k;
        if ((k & (OPS_PER_WORD - 1)) == 0) { sink(k / OPS_PER_WORD - 1, acc); acc = 0; }
    }
    if (k & (OPS_PER_WORD - 1)) sink(k / OPS_PER_WORD, acc);
    const int err = w.finish_counted(out) | overrun;
    head[0] = w.nsteps; head[1] = c0 + w.col; head[2] = w.row; head[3] = w.nopen;
    return err;
}

}  // namespace pcpath
