// pc_prefilter_plan.h -- the table plan of the exact prefilter (pc_prefilter.hip), built on the host.
//
// Everything the prefilter's kernels read that depends on the adapter list and its edit bounds is decided here: how the
// adapters are cut into pieces of at most 32 bases, how the pieces are packed into launches of 8, 4, 2 or 1 per lane, which
// pieces the seed stage takes and with which seed length, and every table word of both stages.  No HIP, no environment, no
// context: pc_api.cpp uploads a Plan and launches over it; tests/host/test_prefilter_plan.cpp interprets one on the CPU
// against the oracle.  These rules decide whether a cleared mask bit is still a proof.
//
// Which read codes an adapter row matches is pc_letters.h.  With IUPAC wildcards (`wildcards`, the context's mode) a row's Eq bit
// is set for every base of its set and for nothing else; an edit is then a column that is not a match under that rule, which is
// what max_edits bounds.  A piece that holds a degenerate letter has no seeds.  On the plane a read's non-base is held as 'A'
// and so matches every row whose set holds A: more matches than the rule gives, never fewer -- a cleared bit stays a proof.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pc_letters.h"

namespace pcp {

// the reference's Dna5 ordinals: everything that is not A/C/G/T(U) is N
inline int dna5(unsigned char c)
{
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 4;
    }
}

// pc_prefilter_max_edits (include/porechop_amd.h).
// A hit has full-adapter identity 100 M / L >= threshold after the reference's %f rounding (six decimals;
// alignment.cpp:113-121 -> nanopore_read.py:476-491), L = alignment columns from the adapter's first to its
// last base, M <= adapter_len of them matches.  With tau = (threshold - 1e-6) / 100:  M >= tau L,  so the
// e = L - M non-matching columns -- each one unit-cost edit between the adapter and the read bases under its
// span -- number at most M (1 - tau) / tau <= adapter_len (1 - tau) / tau.
inline int max_edits(int adapter_len, double threshold_percent)
{
    if (adapter_len <= 0) return -1;
    const double tau = (threshold_percent - 1e-6) / 100.0;
    if (!(tau > 0.0)) return adapter_len;                 // everything is a hit: nothing can be excluded
    if (tau >= 1.0) return 0;
    const double e = (double)adapter_len * (1.0 - tau) / tau;
    const int k = (int)floor(e + 1e-9);                   // + 1e-9: never round a bound DOWN across an integer
    return k > adapter_len ? adapter_len : k;
}

// Where the reads come from and which stages may run.  The seed tables differ between bytes and plane (q-gram orientation
// and base codes); the exhaustive tables between the two routes over the plane ([256][P] rows per group, never launched on
// PlaneSeeds, or [4][P] with wildcards).
enum class Route { Bytes = 0, PlaneSeeds = 1, PlaneTotal = 2 };

struct Options {
    bool no_seeds = false;          // every piece runs the exhaustive kernel
    bool force_multi_q = false;     // a bitmap per seed length, whatever the candidate rates
    bool force_single_q = false;    // one seed length for all pieces, whatever the candidate rates
};

struct Launch { int P, groups; size_t table_off, meta_off; };     // one kernel launch: `groups` groups of P pieces

// 4^8 bits for the longest seed length, then 4^7, then 4^6 (pck::kSeedBitmapWords)
constexpr int kBitmapWords = (1 << 16) / 32 + (1 << 14) / 32 + (1 << 12) / 32;

struct Plan {
    // exhaustive kernel: Eq words [group][256 byte values or 4 codes][P] and [group][P][4] metadata (len, k, mask word,
    // mask bit) of every launch below, the rest launches' behind the others'
    std::vector<uint32_t> tables;
    std::vector<int32_t> meta;
    std::vector<Launch> launches;         // over ALL pieces (no seed stage, or its candidate list overflowed)
    std::vector<Launch> rest_launches;    // over the pieces the seed stage cannot take; only filled when nq > 0
    int warm = 0;                         // longest piece + its bound: the columns scanned before a chunk
    // seed stage
    int nq = 0, q[3] = {6, 6, 6}, first_off[3] = {0, 0, 0}, npieces = 0;     // seed lengths present, longest first; seeded pieces
    double rate = 0.0;                    // expected candidates per read column
    std::vector<uint32_t> bitmaps, first, piece_eq;
    std::vector<int32_t> entries, piece_meta;
    bool seeds_only = false;              // Route::PlaneSeeds can take this list: something is seeded and nothing is left over
};

struct Piece { int adapter, begin, len, k, word; uint32_t bit; };

// A piece of len bases with bound k is cut into k + 1 parts of floor/ceil(len / (k + 1)) bases; it can be seeded when
// those parts are at least 6 bases long and k + 1 <= 8.  Its own seed length is min(8, floor(len / (k + 1))).
inline bool seedable(const Piece &pc, int *q)
{
    const int parts = pc.k + 1;
    *q = std::min(8, pc.len / std::max(1, parts));
    return pc.k >= 0 && pc.k < pc.len && parts <= 8 && *q >= 6;
}

// Eq words of Dna5 codes 0..4: the piece in the TOP bits (row r at bit 32 - len + r), the bits below it match-all
inline void eq_words(const std::string &ad, const Piece &pc, uint32_t out[5], bool wildcards = false)
{
    const uint32_t wild = pc.len >= 32 ? 0u : (0xFFFFFFFFu >> pc.len);
    for (int code = 0; code < 5; ++code) {
        uint32_t e = wild;
        for (int r = 0; r < pc.len; ++r)
            if (pcl::matches(pcl::letter_set((uint8_t)ad[pc.begin + r], wildcards), code)) e |= 1u << (32 - pc.len + r);
        out[code] = e;
    }
}

// Groups of 8 pieces per lane, the remainder r as one smaller group where an unused slot would cost more than a second
// pass over the reads (r = 5 -> 4 + 1, r = 6 -> 4 + 2; r = 3 -> 4, r = 7 -> 8 with a slot idle).  emit(first, count, P).
template <typename Emit>
inline void split_groups(size_t n, Emit emit)
{
    const size_t n8 = n / 8 * 8, r = n - n8;
    if (n8) emit((size_t)0, n8, 8);
    switch (r) {
        case 0: break;
        case 1: emit(n8, (size_t)1, 1); break;
        case 2: emit(n8, (size_t)2, 2); break;
        case 3: case 4: emit(n8, r, 4); break;
        case 5: emit(n8, (size_t)4, 4); emit(n8 + 4, (size_t)1, 1); break;
        case 6: emit(n8, (size_t)4, 4); emit(n8 + 4, (size_t)2, 2); break;
        default: emit(n8, r, 8); break;
    }
}

// Appends the launches over `list` and their tables to the plan.
inline void add_groups(const std::vector<std::string> &adapters, const std::vector<Piece> &list, Route route,
                       std::vector<Launch> &launches, Plan &out, bool wildcards = false)
{
    const size_t rows = route == Route::PlaneTotal ? 4 : 256;        // Eq rows per group: one per 2-bit code / per byte value
    split_groups(list.size(), [&](size_t first, size_t count, int P) {
        const int groups = (int)((count + P - 1) / P);
        const Launch L{P, groups, out.tables.size(), out.meta.size()};
        out.tables.resize(out.tables.size() + (size_t)groups * rows * P, 0xFFFFFFFFu);          // unused slots: all wildcards
        out.meta.resize(out.meta.size() + (size_t)groups * P * 4, 0);
        for (size_t i = 0; i < count; ++i) {
            const Piece &pc = list[first + i];
            const size_t g = i / P, slot = i % P;
            const uint32_t wild = pc.len >= 32 ? 0u : (0xFFFFFFFFu >> pc.len);     // the bits below the piece
            uint32_t eq[5];
            eq_words(adapters[pc.adapter], pc, eq, wildcards);
            if (route == Route::PlaneTotal) {
                // the plane holds codes 0..3 only, a read's non-base among them as 0: an adapter letter that is not a
                // base (Dna5 code 4) matches all four, so that no match of the byte route (N == N) is lost.  (With wildcards
                // eq[4] holds no row: a row matches exactly the bases of its set.)
                for (size_t code = 0; code < 4; ++code) out.tables[L.table_off + (g * 4 + code) * P + slot] = eq[code] | (eq[4] & ~wild);
            } else {
                for (int b = 0; b < 256; ++b) out.tables[L.table_off + (g * 256 + b) * P + slot] = eq[dna5((unsigned char)b)];
            }
            int32_t *mt = &out.meta[L.meta_off + (g * P + slot) * 4];
            mt[0] = pc.len; mt[1] = pc.k; mt[2] = pc.word; mt[3] = (int32_t)pc.bit;
        }
        launches.push_back(L);
    });
}

// The plan of adapters[ids[j]] with bound max_edits[j] (< 0: do not filter this adapter), j < n; bit j % 32 of mask word
// j / 32 is adapter j's.  Returns 0, or -1 for an adapter index outside `adapters` (then `out` is unspecified).
inline int build(const std::vector<std::string> &adapters, const int32_t *ids, const int32_t *max_edits, int n, Route route,
                 const Options &opt, Plan &out, bool wildcards = false)
{
    out = Plan();
    const bool plane = route != Route::Bytes;
    // Pieces.  An adapter of at most 32 bases is one piece with its own bound.  A longer one that allows at most 8
    // edits is represented by its FIRST 32 BASES with the same bound (within k edits of a substring, so is every
    // substring of it: still a proof, and a 32-mer within <= 8 edits of random text is rare).  Beyond that it is cut
    // into p = ceil(m / 32) pieces of nearly equal length, one of which lies within floor(k / p) (pigeonhole).
    std::vector<Piece> pieces;
    for (int j = 0; j < n; ++j) {
        const int ai = ids[j];
        if (ai < 0 || ai >= (int)adapters.size()) return -1;
        const int m = (int)adapters[ai].size();
        if (m <= 0) continue;                                     // an empty adapter never hits (failure record)
        const int k = max_edits[j] < 0 ? m : max_edits[j];
        if (m > 32 && k <= 8) {
            pieces.push_back({ai, 0, 32, k, j / 32, 1u << (j % 32)});
            out.warm = std::max(out.warm, 32 + k);
            continue;
        }
        const int np = (m + 31) / 32;
        int pos = 0;
        for (int t = 0; t < np; ++t) {
            const int len = m / np + (t < m % np ? 1 : 0);
            pieces.push_back({ai, pos, len, k / np, j / 32, 1u << (j % 32)});
            out.warm = std::max(out.warm, len + k / np);
            pos += len;
        }
    }
    add_groups(adapters, pieces, route, out.launches, out, wildcards);

    // ---- seed stage: which pieces it takes, and its tables ------------------------------------------------------
    // ONE seed length for all pieces -- the shortest any seedable piece needs: a longer part's seed is its first q bases, which
    // an occurrence that leaves the part untouched contains just the same.  The scan then probes one bitmap per read base
    // instead of one per length; the price is more candidates for the verifier (an 8-base seed cut to 7 is found four times
    // as often).  That pays for a handful of adapters and not for a barcode panel: one length only while
    // the expected candidate rate stays below 2e-3 per base or within 1.5 x of the per-length rate, unless an option forces.
    int q_common = 8, q = 0;
    for (const Piece &pc : pieces)
        if (seedable(pc, &q)) q_common = std::min(q_common, q);
    double rate_multi = 0.0, rate_single = 0.0;
    for (const Piece &pc : pieces)
        if (seedable(pc, &q)) {
            rate_multi += (double)(pc.k + 1) / (double)(1u << (2 * q));
            rate_single += (double)(pc.k + 1) / (double)(1u << (2 * q_common));
        }
    const bool multi_q = opt.force_multi_q || (!opt.force_single_q && rate_single > 2e-3 && rate_single > 1.5 * rate_multi);
    struct Seed { int cls; uint32_t gram; int piece, off; };     // cls: the seed length until the lengths present are known
    std::vector<Seed> seeds;
    std::vector<Piece> seeded, rest;
    bool have_q[9] = {false, false, false, false, false, false, false, false, false};
    for (const Piece &pc : pieces) {
        const std::string &ad = adapters[pc.adapter];
        bool ok = seedable(pc, &q) && !opt.no_seeds;
        if (ok && !multi_q) q = q_common;
        // on the plane a letter that is not a base ANYWHERE in the adapter leaves the piece to the exhaustive kernel (an 'N'
        // of the adapter would match the read's 'N', which the plane holds as 'A')
        if (ok && plane)
            for (char ch : ad) if (dna5((unsigned char)ch) > 3) ok = false;
        // wildcards: a piece that holds a degenerate letter has no seeds (a seed is one exact q-gram)
        if (ok && wildcards)
            for (int r = 0; r < pc.len; ++r) if (pcl::degenerate((uint8_t)ad[pc.begin + r])) ok = false;
        const size_t seeds_before = seeds.size();
        const int parts = pc.k + 1;
        int pos = 0;
        for (int t = 0; t < parts && ok; ++t) {
            // byte route: the seed scan's code of a base is bits 1-2 of its ASCII byte (A 0, C 1, T/U 2, G 3; either case),
            // first base in the HIGHEST bits; plane: the Dna ordinals, first base in the LOWEST
            uint32_t gram = 0;
            for (int r = 0; r < q && ok; ++r) {
                const unsigned char ch = (unsigned char)ad[pc.begin + pos + r];
                if (dna5(ch) > 3) ok = false;                    // every seed is made of A/C/G/T
                else if (plane) gram |= (uint32_t)dna5(ch) << (2 * r);
                else gram = (gram << 2) | (((uint32_t)ch >> 1) & 3u);
            }
            seeds.push_back({q, gram, (int)seeded.size(), pos});
            pos += pc.len / parts + (t < pc.len % parts ? 1 : 0);
        }
        if (ok) {
            have_q[q] = true;
            seeded.push_back(pc);
        } else {
            seeds.resize(seeds_before);
            rest.push_back(pc);
        }
    }
    int cls_of_q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 8; t >= 6; --t) if (have_q[t]) { cls_of_q[t] = out.nq; out.q[out.nq++] = t; }
    out.npieces = (int)seeded.size();
    out.seeds_only = out.nq > 0 && rest.empty();
    if (out.nq > 0) {
        out.bitmaps.assign(kBitmapWords, 0u);
        const int bm_off[3] = {0, (1 << 16) / 32, (1 << 16) / 32 + (1 << 14) / 32};
        for (Seed &sd : seeds) sd.cls = cls_of_q[sd.cls];
        std::stable_sort(seeds.begin(), seeds.end(), [](const Seed &x, const Seed &y) { return x.cls != y.cls ? x.cls < y.cls : x.gram < y.gram; });
        // per class a [4^q + 1] table of entry ranges; entries: piece, offset of the seed in the piece, 0, 0
        out.entries.assign(seeds.size() * 4 + 4, 0);
        size_t e = 0;
        for (int cl = 0; cl < out.nq; ++cl) {
            const uint32_t ngram = 1u << (2 * out.q[cl]);
            out.first_off[cl] = (int)out.first.size();
            out.first.resize(out.first.size() + ngram + 1, 0u);
            uint32_t *f = out.first.data() + out.first_off[cl];
            for (uint32_t g = 0; g < ngram; ++g) {
                f[g] = (uint32_t)e;
                while (e < seeds.size() && seeds[e].cls == cl && seeds[e].gram == g) {
                    out.entries[e * 4] = seeds[e].piece; out.entries[e * 4 + 1] = seeds[e].off;
                    out.bitmaps[bm_off[cl] + (g >> 5)] |= 1u << (g & 31);
                    ++e;
                }
            }
            f[ngram] = (uint32_t)e;
            out.rate += (double)(f[ngram] - f[0]) / (double)ngram;
        }
        out.piece_meta.assign((size_t)out.npieces * 4 + 4, 0);
        out.piece_eq.assign((size_t)out.npieces * 8 + 8, 0u);
        for (int i = 0; i < out.npieces; ++i) {
            const Piece &pc = seeded[i];
            int32_t *mt = &out.piece_meta[(size_t)i * 4];
            mt[0] = pc.len; mt[1] = pc.k; mt[2] = pc.word; mt[3] = (int32_t)pc.bit;
            eq_words(adapters[pc.adapter], pc, &out.piece_eq[(size_t)i * 8], wildcards);
        }
        // the rest (long pieces with large bounds, tiny adapters, seeds with an N) keeps the exhaustive kernel:
        // its groups are appended to the same tables
        add_groups(adapters, rest, route, out.rest_launches, out, wildcards);
    }
    if (out.tables.empty()) { out.tables.assign(4, 0); out.meta.assign(4, 0); }
    return 0;
}

}  // namespace pcp
