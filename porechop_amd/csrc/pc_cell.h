// pc_cell.h -- ONE cell of the reference's recurrence in plain int32, with what goes round it: the -inf of its gap
// states, the Dna5 code of a byte, the scout that picks the end cell, and the record of a failed alignment.  Written once
// for device and host; pcs::align_pair (pc_slow.h: one trace byte per cell) and pcpath::align_path_window (pc_paths.h:
// packed trace, the path handed back) are its two callers, and the only two places that walk a plain-int32 DP.
//
// The recurrence, tie rules, scout order and _correctTraceValue are SURVEY.md 8a-2..a-4 read literally
// (seqan/align/dp_formula_affine.h:456-495, dp_formula_linear.h:150-182, dp_scout.h:165-179,
// dp_algorithm_impl.h:1352-1369).  Affine when gap_open != gap_extend, the reference's linear-gap dispatch otherwise
// (global_alignment_unbanded.h:217-220).  The trace is kept as the nibble pc_walk.h consumes.
#pragma once
#include <limits.h>
#include <stdint.h>

#include "pc_walk.h"

namespace pcc {

constexpr int NEG_INF = INT_MIN / 2;        // seqan/align/dp_cell.h:116-124

PC_HD int dna5_code(uint8_t c)
{
    // seqan/basic/alphabet_residue_tabs.h:113-140
    if (c == 'A' || c == 'a') return 0;
    if (c == 'C' || c == 'c') return 1;
    if (c == 'G' || c == 'g') return 2;
    if (c == 'T' || c == 't' || c == 'U' || c == 'u') return 3;
    return 4;
}

// an empty read or adapter -- alignment.cpp:9-21: only field 0 and the score are defined
PC_HD void failure_record(pcw::Digest &out)
{
    out.read_start = -1; out.read_end = 0; out.adapter_start = -1; out.adapter_end = 0; out.score = INT_MIN;
    out.matches = 0; out.aligned_len = 0; out.full_len = 0;
}

struct Cell { int S, Hs, Vs, nib; };      // M, H and V of the cell (H = V = -inf in the linear dispatch), its trace nibble

// diag, upM, upV: M of (i - 1, j - 1), M and V of (i - 1, j); Mi = M of (i, j - 1); H: the column state's H(i), still
// that of column j - 1 -- read and written in the affine dispatch only; sub: the score of the two bases.
PC_HD Cell cell(bool linear, int diag, int sub, int upM, int upV, int Mi, int &H, int gap_open, int gap_extend)
{
    Cell c;
    c.Hs = NEG_INF; c.Vs = NEG_INF;
    if (linear) {
        // strict '<' against vertical, then against horizontal: ties prefer diagonal, then vertical; every gap step is a
        // step of its own (both open bits set: pc_walk.h then never runs a gap)
        c.S = diag + sub; c.nib = pcw::NIB_HOPEN | pcw::NIB_VOPEN;
        int t = upM + gap_extend;
        if (c.S < t) { c.S = t; c.nib |= pcw::NIB_NOTDIAG; }
        t = Mi + gap_extend;
        if (c.S < t) { c.S = t; c.nib |= pcw::NIB_NOTDIAG | pcw::NIB_FROMH; }
    } else {
        // strict '<' throughout: a gap is extended rather than opened, V is preferred to H, the diagonal to both
        c.nib = 0;
        c.Hs = H + gap_extend;
        int t = Mi + gap_open;
        if (c.Hs < t) { c.Hs = t; c.nib |= pcw::NIB_HOPEN; }
        c.Vs = upV + gap_extend;
        t = upM + gap_open;
        if (c.Vs < t) { c.Vs = t; c.nib |= pcw::NIB_VOPEN; }
        c.S = c.Vs;
        if (c.S < c.Hs) { c.S = c.Hs; c.nib |= pcw::NIB_FROMH; }
        const int d = diag + sub;
        if (c.S <= d) c.S = d; else c.nib |= pcw::NIB_NOTDIAG;
        H = c.Hs;
    }
    return c;
}

// The end cell: the best M among the cells offered, in visiting order (column by column, down each column) with a strict
// '>', from 0 at (m, 0).  The callers offer the cells of the last row and of the read's last column.
struct Scout {
    int M, H, V, I, J;
    PC_HD void start(int m) { M = 0; H = NEG_INF; V = NEG_INF; I = m; J = 0; }
    PC_HD void offer(const Cell &c, int i, int j) { if (c.S > M) { M = c.S; H = c.Hs; V = c.Vs; I = i; J = j; } }
    // _correctTraceValue, for pcw::Walk::start (affine only; at (m, 0) H = V = -inf != M)
    PC_HD int tie_fix(bool linear) const { return linear ? 0 : (V == M) ? 1 : (H == M) ? 2 : 0; }
};

}  // namespace pcc
