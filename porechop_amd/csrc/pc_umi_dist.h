// pc_umi_dist.h -- the unit-cost edit distance of two UMI keys, bit-parallel, and the bound that settles a pair without it.
//
// KEY.  Up to 64 bases as two bit planes and a length 0 .. 64.  Base t has code c (A C G T/U = 0 1 2 3): bit t of p0 is
// c & 1, bit t of p1 is c >> 1.  Bits at and above the length are ignored: every routine masks them.  The four match masks
// of a key are four operations (~p1 & ~p0, ~p1 & p0, p1 & ~p0, p1 & p0, each under the length mask), its base composition
// four popcounts.
//
// DISTANCE.  distance<Word>(a, la, b, lb): Levenshtein's distance by Myers' bit vectors in Hyyro's form for the GLOBAL
// distance.  The rows are the bases of a (bit r = row r), one column per base of b.  Pv / Mv hold the vertical deltas +1 / -1
// of the column; per column
//     Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;  Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
//     score += bit la-1 of Ph;  score -= bit la-1 of Mh
//     Ph = (Ph << 1) | 1;  Mh <<= 1;  Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv
// The | 1 is the horizontal +1 of the top boundary row (D[0][j] = j); the score starts at la (D[la][0]).  The carry of the
// addition only travels upwards, so what stands in the bits above la never reaches bit la - 1.  la == 0 gives lb.  Word is
// uint32_t when both lengths are <= 32, uint64_t otherwise.
//
// LOWER BOUND.  lower_bound(a, la, b, lb) = max(|la - lb|, S+, S-) with S+ = sum over the four bases c of
// max(0, n_a[c] - n_b[c]) and S- the same with a and b exchanged.  It never exceeds the distance.  Proof: take an optimal
// edit script from a to b.  S+ counts the bases a holds in surplus; every unit of it must leave: a deletion removes one
// base of a, a substitution changes one base of a into another -- either lowers S+ by at most one, an insertion by none.
// After the script the surplus is 0, so the script has at least S+ edits.  The same with the roles exchanged gives S-, and
// the length changes by at most one per edit, which gives |la - lb|.  Since S+ - S- = la - lb and S+ + S- = SAD, the sum of
// the four |n_a[c] - n_b[c]|, the maximum of the three is (SAD + |la - lb|) / 2, exactly (SAD and la - lb have one parity,
// and |la - lb| <= SAD): lower_bound_packed computes that from compositions packed one count to a byte.
//
// MIRROR.  mirror(k, len) is the key of the reverse complement: base t of the result is 3 - base(len - 1 - t).  A molecule read
// from its other strand shows the key START+END as rc(END)+rc(START), which is mirror() of the concatenation.  Both planes are
// bit-reversed within len and inverted under the length mask (3 - c flips both bits of c); len 0 gives the empty key, and
// mirror(mirror(k)) = k under the mask.  Reversal and complement are both isometries of the edit distance, so
// d(a, mirror(b)) = d(mirror(a), b).  mirror_composition(comp) is the composition of the mirrored key: the counts of A and T and
// of C and G change places, and since composition() packs one count to a byte in the order A C G T (A in the lowest byte), that
// is the reversal of the word's four bytes.  lower_bound_packed(composition(a), la, mirror_composition(composition(b)), lb) is
// a lower bound on d(a, mirror(b)): mirror(b) has length lb and that composition, and the proof above is about any two keys --
// apply it to a and mirror(b).
//
// Plain C++ for the host and the device: no runtime include, usable from pc_umi_groups.hip and tests/host/test_umi_dist.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCUD_HD __host__ __device__ inline
#else
#define PCUD_HD inline
#endif

namespace pcud {

constexpr int MAX_LEN = 64;

struct Key { uint64_t p0, p1; };

// ones in bits 0 .. len - 1 (len 0 .. 64)
PCUD_HD uint64_t len_mask(int len)
{
    return len >= 64 ? ~(uint64_t)0 : (len <= 0 ? (uint64_t)0 : (((uint64_t)1 << len) - 1));
}

PCUD_HD int popcount64(uint64_t x) { return __builtin_popcountll(x); }

// the rows of key k (len bases) that hold base c, as a Word
template <typename Word>
PCUD_HD Word match_mask(Key k, int len, int c)
{
    const uint64_t a = (c & 1) ? k.p0 : ~k.p0, b = (c & 2) ? k.p1 : ~k.p1;
    return (Word)(a & b & len_mask(len));
}

// the base of column t of key k
PCUD_HD int base_at(Key k, int t)
{
    return (int)((k.p0 >> t) & 1u) | ((int)((k.p1 >> t) & 1u) << 1);
}

// one column of the recurrence over the match mask Eq of the column's base; top = la - 1, the bit of the last row
template <typename Word>
PCUD_HD void column(Word Eq, int top, Word &Pv, Word &Mv, int &score)
{
    const Word Xv = Eq | Mv;
    const Word Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    Word Ph = Mv | ~(Xh | Pv);
    Word Mh = Pv & Xh;
    score += (int)((Ph >> top) & 1u) - (int)((Mh >> top) & 1u);
    Ph = (Word)(Ph << 1) | (Word)1;
    Mh = (Word)(Mh << 1);
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}

template <typename Word>
PCUD_HD int distance(Key a, int la, Key b, int lb)
{
    if (la == 0) return lb;
    const Word eq[4] = {match_mask<Word>(a, la, 0), match_mask<Word>(a, la, 1), match_mask<Word>(a, la, 2), match_mask<Word>(a, la, 3)};
    const int top = la - 1;
    Word Pv = (Word)len_mask(la), Mv = 0;
    int score = la;
    for (int t = 0; t < lb; ++t) column<Word>(eq[base_at(b, t)], top, Pv, Mv, score);
    return score;
}

// the width the kernel would take for the pair
PCUD_HD int distance_any(Key a, int la, Key b, int lb)
{
    return (la <= 32 && lb <= 32) ? distance<uint32_t>(a, la, b, lb) : distance<uint64_t>(a, la, b, lb);
}

// the four base counts of a key, one to a byte (A in the lowest): each 0 .. 64
PCUD_HD uint32_t composition(Key k, int len)
{
    const uint64_t m = len_mask(len);
    const uint32_t n1 = (uint32_t)popcount64(~k.p1 & k.p0 & m), n2 = (uint32_t)popcount64(k.p1 & ~k.p0 & m),
                   n3 = (uint32_t)popcount64(k.p1 & k.p0 & m);
    return ((uint32_t)len - n1 - n2 - n3) | (n1 << 8) | (n2 << 16) | (n3 << 24);
}

// the three terms of the bound: {|la - lb|, S+, S-}
PCUD_HD void lower_bound_terms(Key a, int la, Key b, int lb, int term[3])
{
    const uint32_t ca = composition(a, la), cb = composition(b, lb);
    int plus = 0, minus = 0;
    for (int c = 0; c < 4; ++c) {
        const int d = (int)((ca >> (8 * c)) & 255u) - (int)((cb >> (8 * c)) & 255u);
        if (d > 0) plus += d; else minus -= d;
    }
    term[0] = la > lb ? la - lb : lb - la;
    term[1] = plus;
    term[2] = minus;
}

PCUD_HD int lower_bound(Key a, int la, Key b, int lb)
{
    int t[3];
    lower_bound_terms(a, la, b, lb, t);
    const int m = t[1] > t[2] ? t[1] : t[2];
    return t[0] > m ? t[0] : m;
}

// the same value from the packed compositions: (SAD + |la - lb|) / 2
PCUD_HD int lower_bound_packed(uint32_t ca, int la, uint32_t cb, int lb)
{
    int sad = 0;
    for (int c = 0; c < 4; ++c) {
        const int d = (int)((ca >> (8 * c)) & 255u) - (int)((cb >> (8 * c)) & 255u);
        sad += d < 0 ? -d : d;
    }
    return (sad + (la > lb ? la - lb : lb - la)) >> 1;
}

// the 64 bits of x in reverse order
PCUD_HD uint64_t reverse64(uint64_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(x);
#endif
}

// the key of the reverse complement: base t is 3 - base(len - 1 - t); the bits at and above len are 0
PCUD_HD Key mirror(Key k, int len)
{
    Key r = {0, 0};
    if (len <= 0) return r;
    if (len > 64) len = 64;
    const uint64_t m = len_mask(len);
    r.p0 = ~(reverse64(k.p0) >> (64 - len)) & m;
    r.p1 = ~(reverse64(k.p1) >> (64 - len)) & m;
    return r;
}

// composition() of the mirrored key: A <-> T and C <-> G, i.e. the four count bytes (A C G T from the lowest) in reverse order
PCUD_HD uint32_t mirror_composition(uint32_t comp) { return __builtin_bswap32(comp); }

}  // namespace pcud
