// pc_paths.h -- one alignment in plain int32 coordinates that hands back its PATH: the digest every kernel of this
// library writes, a four-int head and the path's operations, two bits each.  Written once for device (pc_paths.hip:
// one lane per pair) and host (tests/host/test_paths.cpp replays every path base by base against the oracle).
//
// The recurrence, tie rules, scout order and _correctTraceValue are those of pcs::align_pair (pc_slow.h), restated:
// SURVEY.md 8a-2..a-4 read literally (seqan/align/dp_formula_affine.h:456-495, dp_formula_linear.h:150-182,
// dp_scout.h:165-179, dp_algorithm_impl.h:1352-1369).  Affine when gap_open != gap_extend, the reference's linear-gap
// dispatch otherwise (global_alignment_unbanded.h:217-220).  The traceback and the digest ARE pc_walk.h.
//
// What differs from pc_slow.h is the trace and what the walk leaves behind:
//   * the pc_walk.h nibble is kept PACKED, eight adapter rows to a dword: row i sits in bits 4 ((i - 1) % 8) of the
//     dword of row group (i - 1) / 8.  The dword is built in a register while a column is walked down and stored once
//     per eight rows (and once more for a last, partial group);
//   * every step of the walk is classified from (col, row) before and after Walk::consume and leaves as an operation.
//
// Operations (the adapter plays the role SAM gives the reference, the window that of the query):
//   0 '='  diagonal step over equal Dna5 codes (N == N is equal)      2 'I'  read base against a gap (horizontal step)
//   1 'X'  diagonal step over unequal codes                           3 'D'  adapter base against a gap (vertical step)
// They leave in the order the traceback visits them -- FROM THE END CELL TO THE PATH'S FIRST CELL -- sixteen to a dword,
// the first in the lowest bits; nothing is ever reversed here.  path_cigar() below reads the dwords backwards.
//
// head = {path_len, read_first, adapter_first, opens}: steps of the path, read bases before it (the walk's a), adapter
// bases before it (b; a or b is 0), gap steps that opened their gap (Walk::nopen).
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "pc_walk.h"

namespace pcpath {

constexpr int NEG_INF = INT_MIN / 2;        // seqan/align/dp_cell.h:116-124
enum : int { OP_EQ = 0, OP_X = 1, OP_I = 2, OP_D = 3 };
constexpr int ROWS_PER_WORD = 8, OPS_PER_WORD = 16;

PC_HD int row_groups(int m) { return (m + ROWS_PER_WORD - 1) / ROWS_PER_WORD; }
// dwords that hold the operations of any path over n read bases and m adapter bases (at most n + m steps)
PC_HD int64_t ops_words(int64_t n, int64_t m) { return (n + m + OPS_PER_WORD - 1) / OPS_PER_WORD; }

// Mem:  int &M(int i), int &H(int i)              for adapter rows i = 1..m (the column state)
//       void put(int j, int g, uint32_t word)     the packed trace of column j = 1..n, row group g = 0..row_groups(m)-1
//       uint32_t get(int j, int g)
// rd(k) / ad(k): Dna5 code of the k-th (0-based) read / adapter base.
// sink(k, word): the k-th dword of operations; each is handed out when full, the last (partial) one at the end.
// -> 0, or 1 if the walk reported an inconsistency or did not end within n + m + 8 steps (never expected).
// n or m == 0: the reference's failure record, a zero head, no operations.
template <typename Mem, typename RdFn, typename AdFn, typename Sink>
PC_HD int align_path(int n, int m, RdFn rd, AdFn ad, int match, int mismatch, int gap_open, int gap_extend, Mem mem,
                     pcw::Digest &out, int32_t head[4], Sink sink)
{
    head[0] = 0; head[1] = 0; head[2] = 0; head[3] = 0;
    if (n <= 0 || m <= 0) {                   // alignment.cpp:9-21: only field 0 and the score are defined
        out.read_start = -1; out.read_end = 0; out.adapter_start = -1; out.adapter_end = 0; out.score = INT_MIN;
        out.matches = 0; out.aligned_len = 0; out.full_len = 0;
        return 0;
    }
    const bool linear = gap_open == gap_extend;        // global_alignment_unbanded.h:217-220
    for (int i = 1; i <= m; ++i) { mem.M(i) = 0; mem.H(i) = NEG_INF; }
    int bestM = 0, bestH = NEG_INF, bestV = NEG_INF, bestI = m, bestJ = 0;
    for (int j = 1; j <= n; ++j) {
        int diag = 0, upM = 0, upV = NEG_INF;          // row 0: M = 0, V = -inf
        const int h = rd(j - 1);
        const bool last_col = j == n;
        uint32_t word = 0;
        for (int i = 1; i <= m; ++i) {
            const int Mi = mem.M(i);
            const int sub = (h == ad(i - 1)) ? match : mismatch;
            int S, Hs = NEG_INF, Vs = NEG_INF, nib;
            if (linear) {
                // strict '<' against vertical, then against horizontal: ties prefer diagonal, then vertical; every
                // gap step is a step of its own (both open bits set: pc_walk.h then never runs a gap)
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
    // _correctTraceValue (affine only; at (m, 0) H = V = -inf != M)
    int tie_fix = 0;
    if (!linear) tie_fix = (bestV == bestM) ? 1 : (bestH == bestM) ? 2 : 0;
    pcw::Walk w;
    w.start(bestI, bestJ, m, 0, n, bestM, tie_fix);
    const int cap = n + m + 8;                         // a path has at most n + m steps: a corrupted trace ends here
    int overrun = 0, k = 0;
    uint32_t acc = 0;
    while (!w.done) {
        if (k >= cap) { overrun = 1; break; }
        const int c = w.col, r = w.row;
        const int nib = (int)(mem.get(c, (r - 1) / ROWS_PER_WORD) >> (4 * ((r - 1) & (ROWS_PER_WORD - 1)))) & 15;
        const bool eq = rd(c - 1) == ad(r - 1);
        w.consume(nib, eq);
        const bool dcol = w.col != c, drow = w.row != r;
        const uint32_t op = (dcol && drow) ? (eq ? OP_EQ : OP_X) : (drow ? OP_D : OP_I);
        acc |= op << (2 * (k & (OPS_PER_WORD - 1)));
        ++k;
        if ((k & (OPS_PER_WORD - 1)) == 0) { sink(k / OPS_PER_WORD - 1, acc); acc = 0; }
    }
    if (k & (OPS_PER_WORD - 1)) sink(k / OPS_PER_WORD, acc);
    const int err = w.finish_counted(out) | overrun;
    head[0] = w.nsteps; head[1] = w.col; head[2] = w.row; head[3] = w.nopen;
    return err;
}

// (ops, path_len) -> the FORWARD run-length string ("17=1X4=2I6="), NUL-terminated when it fits.  -> the length it
// needs (without the NUL); nothing beyond buflen bytes is written.  An empty path gives "".
inline int path_cigar(const uint32_t *ops, int path_len, char *buf, size_t buflen)
{
    static const char LETTER[4] = {'=', 'X', 'I', 'D'};
    size_t need = 0;
    auto emit = [&](char ch) { if (buf && need < buflen) buf[need] = ch; ++need; };
    int k = path_len - 1;
    while (k >= 0) {
        const uint32_t op = (ops[k / OPS_PER_WORD] >> (2 * (k % OPS_PER_WORD))) & 3u;
        int run = 0;
        while (k >= 0 && ((ops[k / OPS_PER_WORD] >> (2 * (k % OPS_PER_WORD))) & 3u) == op) { ++run; --k; }
        char digits[12];
        int nd = 0;
        while (run > 0) { digits[nd++] = (char)('0' + run % 10); run /= 10; }
        while (nd > 0) emit(digits[--nd]);
        emit(LETTER[op]);
    }
    if (buf && buflen > 0) buf[need < buflen ? need : buflen - 1] = '\0';
    return (int)need;
}

}  // namespace pcpath
