// pc_mask_rule.h -- which records of a masked read can the mask have changed?  Answered from the records alone.
//
// Phase C (nanopore_read.py:210-243) masks the interval [rs, re) of a read that an adapter hit with '-' and aligns again: the
// adapter that hit, then every adapter after it, against the masked read.  The batched rounds of Pipeline.phase_c hold, per
// dirty read, the record of every adapter against the read's CURRENT masked state; after a mask they would realign all of
// them.  Almost all of those alignments return the record already held.  This header says which ones provably do.
//
// THE GATE.  Every adapter letter is one of A, C, G, T, U (either case), wildcards are off, and mismatch <= match.  Then a
// masked base ('-', Dna5 code 4) scores `mismatch` against every adapter row, and every column [rs, re) of the substitution
// matrix is at or below what it was: a column that held matches and mismatches holds mismatches only, a column that was
// masked before (or held an N) is unchanged.  The DP is monotone in its substitution scores, so every cell's value V'(i, j)
// of the masked read is <= its value V(i, j) before.  Without the gate the claim is false: non-ACGTU bytes code as N, and N
// equals N, so AATGTACTNNNNCAGTTACGTATTGCT against a read holding its concrete copy scores 47 and, once '----' is written
// over the four bases under its N's, 81 (tests/host/test_mask_rule.cpp keeps the case).  With wildcards on the letter sets
// are others, and with mismatch > match a masked column can score above a matching one.
//
// THE CLAIM, under the gate, for the record of one (read, adapter) pair:
//   1. A record whose read interval [read_start, read_end] (fields 0 and 1, inclusive) does not intersect [rs, re) is the
//      record of the masked read too.  Its path avoids the masked columns, so the path's cells keep their values, the end
//      cell among them.  The end cell is the first cell, in the order the scan visits them, that holds the best value: every
//      cell visited earlier was strictly below and can only have fallen, no later cell can now exceed it, so it is chosen
//      again.  At every step of the traceback the predecessor that was chosen keeps its value while its competitors can only
//      have fallen, so the same predecessor is chosen, down to the same first cell.  Every field follows from the path.
//   2. A pair whose best score is below a floor F stays below F: a floored call answers it with "no alignment", as before.
//   3. Hence, in a floored call whose floors are all > 0, a "no alignment" record (field 0 == -1) is stable: the pair was
//      below its floor, or its window is empty (best score 0 < F), and both stay so.  In an unfloored call a -1 record is
//      realigned: nothing here says what it stood for.
// The adapter that hit is always realigned (its own record IS the mask).  Adapters below the read's cursor are never consumed
// again and need nothing.  An empty mask (re <= rs) changes no base and no record.
//
// Plain C++17 for the host and the device: no runtime include, usable from the selection kernel of pc_middle.hip and from
// tests/host/test_mask_rule.cpp, which checks the claim against the oracle.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCM_HD __host__ __device__
#else
#define PCM_HD
#endif

namespace pcm {

// Is this adapter byte one of A, C, G, T, U in either case?
PCM_HD inline bool plain_base(uint8_t byte)
{
    const uint8_t b = (uint8_t)(byte | 0x20);
    return b == 'a' || b == 'c' || b == 'g' || b == 't' || b == 'u';
}

// The gate over one adapter: its letters only.
PCM_HD inline bool adapter_allows(const char *adapter, int len)
{
    if (!adapter || len < 0) return false;
    for (int i = 0; i < len; ++i)
        if (!plain_base((uint8_t)adapter[i])) return false;
    return true;
}

// The gate: may the rule below be applied to a scan of these adapters with these scores?  (gap_open and gap_extend do not
// enter the claim; they are taken so that the gate is asked with the whole scheme, and a later condition on them has a place.)
inline bool gate(const char *const *adapters, const int *lens, int n, int match, int mismatch, int gap_open, int gap_extend, bool wildcards)
{
    (void)gap_open; (void)gap_extend;
    if (wildcards || mismatch > match || n < 0 || (n > 0 && (!adapters || !lens))) return false;
    for (int a = 0; a < n; ++a)
        if (!adapter_allows(adapters[a], lens[a])) return false;
    return true;
}

// Does the record's read interval [read_start, read_end] (inclusive) share a column with the mask [rs, re)?
PCM_HD inline bool touches(int32_t read_start, int32_t read_end, int32_t rs, int32_t re)
{
    return (int64_t)read_start < (int64_t)re && (int64_t)read_end >= (int64_t)rs;
}

// The rule, for one active read that was just masked over [rs, re) and now stands at adapter `cur` (the one that hit): must
// adapter `a`, whose record of this read has fields 0 and 1 = read_start, read_end, be aligned again?
// floored_positive: the scan that made the record, and the one that would make the next, are floored with floors all > 0.
PCM_HD inline bool must_realign(int a, int cur, int32_t read_start, int32_t read_end, int32_t rs, int32_t re, bool floored_positive)
{
    if (a < cur) return false;                           // never consumed again
    if (a == cur) return true;                           // the hit itself
    if (read_start == -1) return !floored_positive;      // claim 3
    if (re <= rs) return false;                          // nothing was masked
    if (read_start < 0 || read_end < read_start) return true;    // not a plain record: nothing is claimed about it
    return touches(read_start, read_end, rs, re);        // claim 1
}

}  // namespace pcm
