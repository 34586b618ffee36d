// pc_middle_paths.h -- which window of its masked read the path of a MIDDLE hit is computed from, and why that is exact.
// Host and device: middle_path_kernel (pc_paths.hip) and tests/host/test_middle_paths.cpp, which compares every windowed
// result with pcpath::align_path over the whole, explicitly masked read.
//
// A middle hit is the alignment of an adapter against the whole trimmed read of n bases, with the read intervals of the
// read's earlier hits replaced by '-' (Dna5 code 4).  Masking is in place, so coordinates never move, and the hit list
// alone rebuilds the read a hit was aligned against.  What the list also gives is the hit's exclusive read end `re`.
//
//   window      the DP runs over global columns c0 + 1 .. c1,  c1 = min(n, re + W),  c0 = max(0, re - window), with W and
//               window of pcb::compute_bounds for the adapter's own length (hit_window()).  A scheme compute_bounds
//               refuses gets the whole read: c0 = 0, c1 = n.
//   start state and scout are those of pcpath::align_path_window (pc_paths.h), the one DP-plus-walk body, which gets
//               (c0, c1) from here.
//   mask        is the caller's rd(k): code 4 for every GLOBAL k inside one of the hit's earlier intervals.
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

}  // namespace pcpath
