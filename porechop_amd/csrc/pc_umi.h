// pc_umi.h -- the read bases that lie under an adapter's degenerate letters (its UMI), from the alignment's PATH.
//
// SPAN.  Under the wildcard rule (pc_letters.h) an adapter row is degenerate when its letter set holds two or more bases.
// The adapter's UMI span is rows u0 .. u1 (0-based, inclusive): the first and the last degenerate row.  Fixed rows between
// two degenerate blocks belong to the span; an adapter without a degenerate row has none.
//
// EXTRACTION.  A path as pc_paths.h leaves it: head = {path_len, read_first, adapter_first, opens} and two-bit operations
// in traceback order (operation path_len - 1 is the path's FIRST step).  Walked forward from (i, j) = (read_first,
// adapter_first):
//   '=' 'X'  consume window column i and adapter row j
//   'I'      consumes column i; it lies BEFORE row j, the next row to be consumed
//   'D'      consumes row j
// Column i belongs to the UMI when a diagonal step consumes it with u0 <= j <= u1, or an 'I' consumes it with
// u0 < j <= u1: an insertion with a span row behind it and one still ahead.  Insertions at either edge of the span are
// outside.  i and j only grow, and after the first such column j > u0 while before the last one j <= u1, so the columns
// form ONE run [first, first + len); len == 0 gives first = -1.
//   covered    diagonal steps with j in the span
//   complete   adapter_first <= u0 and the last row the path consumes is >= u1: no edge of the window clipped the span
//
// QUALIFYING.  qualifies() is the condition under which the per-read reduction of phase B (pc_reduce.hip, reduce_kernel)
// lets a record raise a trim.  The identity is the caller's: the device hands in pck::identity (pc_record.h), the host test
// the oracle's, so there is no second rounding here.
//
// Plain C++17 for the host and the device: no runtime include, usable from pc_paths.hip and from tests/host/test_umi.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCU_HD __host__ __device__ inline
#else
#define PCU_HD inline
#endif

namespace pcu {

// does the letter set (pcl::letter_set(byte, true): bits 0..3 = A C G T) hold two or more bases?
PCU_HD bool degenerate_set(unsigned set)
{
    const unsigned s = set & 15u;
    return (s & (s - 1u)) != 0u;
}

// sets(k): the letter set of adapter row k = 0 .. m - 1.  -> true and the span, or false (u0 = u1 = -1)
template <typename SetFn>
PCU_HD bool span(SetFn sets, int m, int *u0, int *u1)
{
    int a = -1, b = -1;
    for (int k = 0; k < m; ++k)
        if (degenerate_set((unsigned)sets(k))) { if (a < 0) a = k; b = k; }
    *u0 = a; *u1 = b;
    return a >= 0;
}

struct Umi { int32_t first, len, covered, complete; };

// word(k): the k-th dword of the path's operations (sixteen to a dword, the first in the lowest bits), asked for only for
// k < ceil(path_len / 16), from the last one down, each once.
template <typename WordFn>
PCU_HD Umi extract(const int32_t head[4], WordFn word, int u0, int u1)
{
    const int L = head[0];
    int i = head[1], j = head[2];
    const bool from_before = j <= u0;
    Umi r = {-1, 0, 0, 0};
    uint32_t w = 0;
    for (int t = L - 1; t >= 0; --t) {
        if (t == L - 1 || (t & 15) == 15) w = word(t >> 4);
        const unsigned op = (w >> (2 * (t & 15))) & 3u;
        const bool inside = j >= u0 && j <= u1;
        if (op <= 1u) {                                  // '=' / 'X'
            if (inside) { if (r.len == 0) r.first = i; ++r.len; ++r.covered; }
            ++i; ++j;
        } else if (op == 2u) {                           // 'I'
            if (inside && j > u0) { if (r.len == 0) r.first = i; ++r.len; }
            ++i;
        } else {                                         // 'D'
            ++j;
        }
    }
    r.complete = (from_before && j > u1) ? 1 : 0;        // j - 1: the last row the path consumed
    return r;
}

// rec: {rs, re (inclusive), matches, aligned_len} of a scan record (pck::Rec); rule: {end_size, min_trim_size,
// end_threshold} (pc_end_rule); identity(matches, aligned_len): the percent identity as phase B sees it.
template <typename Rec, typename Rule, typename IdentityFn>
PCU_HD bool qualifies(const Rec &rec, int side, const Rule &rule, IdentityFn identity)
{
    if (rec.rs < 0) return false;
    const double partial = identity(rec.matches, rec.aligned_len);
    const int rs = rec.rs, re = rec.re + 1;
    if (!(partial > rule.end_threshold) || re - rs < rule.min_trim_size) return false;
    return side == 0 ? re != rule.end_size : rs != 0;
}

}  // namespace pcu
