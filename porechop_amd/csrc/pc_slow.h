// pc_slow.h -- one alignment in PLAIN int32 coordinates, for what the packed 16-bit kernels refuse: scoring schemes
// outside pcb::scores_supported (non-negative gap scores, match <= mismatch, magnitudes beyond the 16-bit lanes) and
// adapters longer than pcb::MAX_ADAPTER.  The reference accepts any four integers and any adapter
// (porechop/porechop.py:145,196-202, porechop/src/adapter_align.cpp:11-31); this is the path that keeps the drop-in
// boundary total.  Written once for device (pc_slow.hip: one LANE per pair, column state and trace in HBM, lane-
// interleaved) and host (tests/host/test_slow.cpp runs this very code against the oracle on unrestricted schemes).
//
// The cell, the scout and _correctTraceValue are pc_cell.h (the one copy, with the reference's lines cited there); the
// trace is kept as the nibble pc_walk.h consumes and the traceback + digest ARE pc_walk.h (matches counted from the
// bases: finish_counted).  No drift, no bounds, no pruning: O(n m) cells, one byte of trace per cell.
//
// Whether two bases match is pc_letters.h: the adapter side is a SET of read codes per row (align_pair_sets; with IUPAC
// wildcards a letter's set of bases); align_pair takes Dna5 codes and is the same body over one-code sets -- the form the host
// programs that hold this file to the oracle call.
#pragma once
#include <stdint.h>

#include "pc_cell.h"
#include "pc_letters.h"

namespace pcs {

// Largest |score| and longest adapter this path takes; the caller also checks (n + m) * max|score| < 2^30 so that no
// sum leaves int32 (the reference's own arithmetic is int: beyond that it is undefined there too).
constexpr int MAX_ABS_SCORE = 1 << 20;
constexpr int MAX_ADAPTER = 4096;

PC_HD bool fits(int n, int m, int match, int mismatch, int gap_open, int gap_extend)
{
    auto ab = [](int x) { return x < 0 ? -(long long)x : (long long)x; };
    long long mx = ab(match);
    if (ab(mismatch) > mx) mx = ab(mismatch);
    if (ab(gap_open) > mx) mx = ab(gap_open);
    if (ab(gap_extend) > mx) mx = ab(gap_extend);
    return mx <= MAX_ABS_SCORE && m <= MAX_ADAPTER && ((long long)n + m + 2) * mx < (1ll << 30);
}

// Mem:  int &M(int i), int &H(int i)   for adapter rows i = 1..m (the column state)
//       uint8_t &T(int j, int i)       trace nibble of cell (column j = 1..n, row i = 1..m)
// rd(k): Dna5 code of the k-th (0-based) read base.  ad(k): the set of read codes the k-th adapter letter matches
// (pcl::letter_set).
// -> 0, or 1 if the walk reported an inconsistency (never expected).  n or m == 0: the reference's failure record.
template <typename Mem, typename RdFn, typename AdFn>
PC_HD int align_pair_sets(int n, int m, RdFn rd, AdFn ad, int match, int mismatch, int gap_open, int gap_extend, Mem mem,
                     pcw::Digest &out)
{
    if (n <= 0 || m <= 0) { pcc::failure_record(out); return 0; }
    const bool linear = gap_open == gap_extend;
    for (int i = 1; i <= m; ++i) { mem.M(i) = 0; mem.H(i) = pcc::NEG_INF; }
    pcc::Scout best;
    best.start(m);
    for (int j = 1; j <= n; ++j) {
        int diag = 0, upM = 0, upV = pcc::NEG_INF;     // row 0: M = 0, V = -inf
        const int h = rd(j - 1);
        const bool last_col = j == n;
        for (int i = 1; i <= m; ++i) {
            const int Mi = mem.M(i);
            const int sub = pcl::matches(ad(i - 1), h) ? match : mismatch;
            const pcc::Cell c = pcc::cell(linear, diag, sub, upM, upV, Mi, mem.H(i), gap_open, gap_extend);
            diag = Mi;
            mem.M(i) = c.S;
            upM = c.S; upV = c.Vs;
            mem.T(j, i) = (uint8_t)c.nib;
            if (last_col || i == m) best.offer(c, i, j);
        }
    }
    pcw::Walk w;
    w.start(best.I, best.J, m, 0, n, best.M, best.tie_fix(linear));
    while (!w.done) {
        const int c = w.col, r = w.row;
        w.consume(mem.T(c, r), pcl::matches(ad(r - 1), rd(c - 1)));
    }
    return w.finish_counted(out);
}

// ad(k): Dna5 code of the k-th adapter base -- the reference's equality, N == N included.
template <typename Mem, typename RdFn, typename AdFn>
PC_HD int align_pair(int n, int m, RdFn rd, AdFn ad, int match, int mismatch, int gap_open, int gap_extend, Mem mem,
                     pcw::Digest &out)
{
    return align_pair_sets(n, m, rd, [&](int k) { return pcl::code_set(ad(k)); }, match, mismatch, gap_open, gap_extend, mem, out);
}

}  // namespace pcs
