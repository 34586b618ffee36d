// pc_paths.h -- one alignment in plain int32 coordinates that hands back its PATH: the digest every kernel of this
// library writes, a four-int head and the path's operations, two bits each -- over the whole read (align_path) or over a
// window of its columns (align_path_window, the one DP-plus-walk body; pc_middle_paths.h says which window).  Written
// once for device (pc_paths.hip: one lane per pair or hit) and host (tests/host/test_paths.cpp replays every path base
// by base against the oracle; tests/host/test_middle_paths.cpp compares every windowed result with align_path over the
// whole, explicitly masked read).
//
// The cell, the scout and _correctTraceValue are pc_cell.h, the copy pcs::align_pair (pc_slow.h) uses too; the
// traceback and the digest ARE pc_walk.h.
//
// What differs from pc_slow.h is the trace and what the walk leaves behind:
//   * the pc_walk.h nibble is kept PACKED, eight adapter rows to a dword: row i sits in bits 4 ((i - 1) % 8) of the
//     dword of row group (i - 1) / 8.  The dword is built in a register while a column is walked down and stored once
//     per eight rows (and once more for a last, partial group);
//   * every step of the walk is classified from (col, row) before and after Walk::consume and leaves as an operation.
//
// Operations (the adapter plays the role SAM gives the reference, the window that of the query):
//   0 '='  diagonal step over a match (pc_letters.h)                  2 'I'  read base against a gap (horizontal step)
//   1 'X'  diagonal step that is not a match                          3 'D'  adapter base against a gap (vertical step)
// A match is pcl::matches(adapter letter's set, read code): with one-code sets equal Dna5 codes (N == N is equal), with
// IUPAC wildcards a read base A/C/G/T inside the adapter letter's set.
// They leave in the order the traceback visits them -- FROM THE END CELL TO THE PATH'S FIRST CELL -- sixteen to a dword,
// the first in the lowest bits; nothing is ever reversed here.  path_cigar() below reads the dwords backwards.
//
// head = {path_len, read_first, adapter_first, opens}: steps of the path, read bases before it (the walk's a), adapter
// bases before it (b; a or b is 0), gap steps that opened their gap (Walk::nopen).
//
// THE WINDOW.  align_path_window runs the DP over global columns c0 + 1 .. c1 of a read of n bases (pc_middle_paths.h says
// which window a middle hit gets, and why the result is exact):
//   start state c0 == 0: the reference's (M(i) = 0, H(i) = -inf).  c0 > 0: the lower-bound state of pc_bounds.h, a row-0
//               start followed by a vertical gap: M(i) = gap_open + (i - 1) * gap_extend, H(i) = -inf (with
//               gap_open == gap_extend that is the linear dispatch's i * gap).
//   scout       the reference's visiting order and strict '>', from (0 at (m, c0)).  The cells of the window's last column
//               are candidates only when that column is the read's last (c1 == n); last-row cells always are.  The end
//               cell is not forced.
// The walk is pcw::Walk with col0 = c0 and n_total = n: the record and head[1] (= c0 + its local column) are in the read's
// coordinates, local columns 1 .. c1 - c0 index the trace, and "left the window" stays an error.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pc_cell.h"
#include "pc_letters.h"

namespace pcpath {

enum : int { OP_EQ = 0, OP_X = 1, OP_I = 2, OP_D = 3 };
constexpr int ROWS_PER_WORD = 8, OPS_PER_WORD = 16;

PC_HD int row_groups(int m) { return (m + ROWS_PER_WORD - 1) / ROWS_PER_WORD; }
// dwords that hold the operations of any path over n read bases and m adapter bases (at most n + m steps)
PC_HD int64_t ops_words(int64_t n, int64_t m) { return (n + m + OPS_PER_WORD - 1) / OPS_PER_WORD; }

// Mem:  int &M(int i), int &H(int i)              for adapter rows i = 1..m (the column state)
//       void put(int j, int g, uint32_t word)     the packed trace of LOCAL column j = 1 .. c1 - c0, row group
//       uint32_t get(int j, int g)                g = 0 .. row_groups(m) - 1
// rd(k): Dna5 code of the k-th (0-based, GLOBAL) base of the (masked) read; only k in [c0, c1) is asked for.
// ad(k): the set of read codes the k-th (0-based) adapter letter matches (pcl::letter_set; pcl::code_set of a Dna5 code).
// sink(k, word): the k-th dword of operations; each is handed out when full, the last (partial) one at the end.
// -> 0, or 1 if the walk reported an inconsistency (leaving the window included) or did not end within c1 - c0 + m + 8
// steps (never expected).  n or m == 0, or an empty window: the reference's failure record, a zero head, no operations.
template <typename Mem, typename RdFn, typename AdFn, typename Sink>
PC_HD int align_path_window_sets(int n, int m, int c0, int c1, RdFn rd, AdFn ad, int match, int mismatch, int gap_open,
                                 int gap_extend, Mem mem, pcw::Digest &out, int32_t head[4], Sink sink)
{
    head[0] = 0; head[1] = 0; head[2] = 0; head[3] = 0;
    const int nc = c1 - c0;
    if (n <= 0 || m <= 0 || nc <= 0) { pcc::failure_record(out); return 0; }
    const bool linear = gap_open == gap_extend;
    if (c0 == 0) for (int i = 1; i <= m; ++i) { mem.M(i) = 0; mem.H(i) = pcc::NEG_INF; }
    else for (int i = 1; i <= m; ++i) { mem.M(i) = gap_open + (i - 1) * gap_extend; mem.H(i) = pcc::NEG_INF; }
    const bool last_is_reads = c1 == n;
    pcc::Scout best;
    best.start(m);
    for (int j = 1; j <= nc; ++j) {
        int diag = 0, upM = 0, upV = pcc::NEG_INF;     // row 0: M = 0, V = -inf
        const int h = rd(c0 + j - 1);
        const bool last_col = last_is_reads && j == nc;
        uint32_t word = 0;
        for (int i = 1; i <= m; ++i) {
            const int Mi = mem.M(i);
            const int sub = pcl::matches(ad(i - 1), h) ? match : mismatch;
            const pcc::Cell c = pcc::cell(linear, diag, sub, upM, upV, Mi, mem.H(i), gap_open, gap_extend);
            diag = Mi;
            mem.M(i) = c.S;
            upM = c.S; upV = c.Vs;
            const int slot = (i - 1) & (ROWS_PER_WORD - 1);
            word |= (uint32_t)c.nib << (4 * slot);
            if (slot == ROWS_PER_WORD - 1 || i == m) { mem.put(j, (i - 1) / ROWS_PER_WORD, word); word = 0; }
            if (last_col || i == m) best.offer(c, i, j);
        }
    }
    pcw::Walk w;
    w.start(best.I, best.J, m, c0, n, best.M, best.tie_fix(linear));
    const int cap = nc + m + 8;                        // a path has at most nc + m steps: a corrupted trace ends here
    int overrun = 0, k = 0;
    uint32_t acc = 0;
    while (!w.done) {
        if (k >= cap) { overrun = 1; break; }
        const int c = w.col, r = w.row;
        const int nib = (int)(mem.get(c, (r - 1) / ROWS_PER_WORD) >> (4 * ((r - 1) & (ROWS_PER_WORD - 1)))) & 15;
        const bool eq = pcl::matches(ad(r - 1), rd(c0 + c - 1));
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

// ad(k): Dna5 code of the k-th adapter base -- the reference's equality, N == N included.
template <typename Mem, typename RdFn, typename AdFn, typename Sink>
PC_HD int align_path_window(int n, int m, int c0, int c1, RdFn rd, AdFn ad, int match, int mismatch, int gap_open,
                            int gap_extend, Mem mem, pcw::Digest &out, int32_t head[4], Sink sink)
{
    return align_path_window_sets(n, m, c0, c1, rd, [&](int k) { return pcl::code_set(ad(k)); }, match, mismatch, gap_open,
                                  gap_extend, mem, out, head, sink);
}

// The alignment against the WHOLE read: the window c0 = 0, c1 = n.  With c0 = 0 the start state is the reference's
// (M(i) = 0, H(i) = -inf), the window's last column is the read's, so its cells are scout candidates as in the
// reference, and head[1] = w.col: every one of the window's differences vanishes, and what is left is the recurrence of
// pcs::align_pair with a packed trace (tests/host/test_paths.cpp holds the three to one another on every case).
// n or m == 0: the reference's failure record, a zero head, no operations.
template <typename Mem, typename RdFn, typename AdFn, typename Sink>
PC_HD int align_path(int n, int m, RdFn rd, AdFn ad, int match, int mismatch, int gap_open, int gap_extend, Mem mem,
                     pcw::Digest &out, int32_t head[4], Sink sink)
{
    return align_path_window(n, m, 0, n, rd, ad, match, mismatch, gap_open, gap_extend, mem, out, head, sink);
}

template <typename Mem, typename RdFn, typename AdFn, typename Sink>
PC_HD int align_path_sets(int n, int m, RdFn rd, AdFn ad, int match, int mismatch, int gap_open, int gap_extend, Mem mem,
                          pcw::Digest &out, int32_t head[4], Sink sink)
{
    return align_path_window_sets(n, m, 0, n, rd, ad, match, mismatch, gap_open, gap_extend, mem, out, head, sink);
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
