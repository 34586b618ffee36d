// The prefilter's table plan (porechop_amd/csrc/pc_prefilter_plan.h), host-compiled and INTERPRETED: what the kernels of
// pc_prefilter.hip compute from a plan is restated here in plain C++ (the textbook form of Myers' recurrence over the plan's
// Eq words, the piece in the top bits) and held against the oracle's edit distance on seeded random cases, for the three
// routes and the four option settings.
//   exhaustive interpreter: every launch, group, slot and column of a window; the piece's bit is set when the score reaches k
//   seed interpreter:       every q-gram of the window, bitmap, first / entries lookup, the verify window, + the rest launches
// Checked per case: the two masks are equal; against pc_oracle_min_edits they are exact (adapters of at most 32 bases; over the
// plane only where read and adapter are made of bases) or a superset (longer adapters, an N over the plane); and the plan's
// structure (each piece in one slot, seeded or rest, idle slots neutral, the seeds-only flag, the candidate rate).
//   usage: test_prefilter_plan [cases [seed]]   ->   bad=0 cases=N seeded=... rest=... long=...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "pc_oracle.h"
#include "pc_prefilter_plan.h"

using pcp::Route;

static long bad = 0, n_seeded = 0, n_rest = 0, n_long = 0;
static unsigned long long g_seed = 20240607ull;
static long g_case = 0;

static void fail(const char *what, Route route, int opt, long a = 0, long b = 0)
{
    if (++bad <= 20) printf("FAIL %s: seed=%llu case=%ld route=%d options=%d (%ld, %ld)\n", what, g_seed, g_case, (int)route, opt, a, b);
}

struct Rng {
    std::mt19937_64 g;
    explicit Rng(unsigned long long s) : g(s) {}
    int below(int n) { return (int)(g() % (unsigned long long)n); }                 // [0, n)
    int in(int lo, int hi) { return lo + below(hi - lo + 1); }                      // [lo, hi]
    bool chance(int percent) { return below(100) < percent; }
    char base() { return "ACGT"[below(4)]; }
    std::string seq(int n) { std::string s; for (int i = 0; i < n; ++i) s.push_back(base()); return s; }
};

// the read as a route's kernels see it: bytes, or the 2-bit plane's letters (a byte that is not a base sits there as 'A')
static std::string view_of(const std::string &read, Route route)
{
    if (route == Route::Bytes) return read;
    std::string v;
    for (char ch : read) v.push_back("ACGTA"[pcp::dna5((unsigned char)ch)]);
    return v;
}

// one column of Myers' recurrence, search variant, the score following the TOP bit (pc_prefilter.hip myers_step)
static void myers_step(uint32_t eq, uint32_t &pv, uint32_t &mv, int &sc)
{
    const uint32_t xv = eq | mv;
    const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint32_t ph = mv | ~(xh | pv), mh = pv & xh;
    sc += (int)(ph >> 31) - (int)(mh >> 31);
    ph <<= 1; mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

// smallest score of a piece of len bases over columns [lo, hi) of the view; eq_of(byte) is the column's Eq word
template <typename EqOf>
static int best_score(const std::string &view, int lo, int hi, int len, EqOf eq_of)
{
    uint32_t pv = len >= 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> len), mv = 0;
    int sc = len, mn = len;
    for (int j = lo; j < hi; ++j) {
        myers_step(eq_of((unsigned char)view[j]), pv, mv, sc);
        mn = std::min(mn, sc);
    }
    return mn;
}

static void exhaustive(const pcp::Plan &p, const std::vector<pcp::Launch> &ls, Route route, const std::string &view, std::vector<uint32_t> &mask)
{
    const size_t rows = route == Route::PlaneTotal ? 4 : 256;
    for (const pcp::Launch &L : ls)
        for (int g = 0; g < L.groups; ++g)
            for (int slot = 0; slot < L.P; ++slot) {
                const int32_t *mt = &p.meta[L.meta_off + ((size_t)g * L.P + slot) * 4];
                if (mt[0] == 0) continue;
                const uint32_t *tab = &p.tables[L.table_off + (size_t)g * rows * L.P + slot];
                const int mn = best_score(view, 0, (int)view.size(), mt[0], [&](unsigned char b) {
                    return tab[(rows == 4 ? (size_t)pcp::dna5(b) : (size_t)b) * L.P];      // (a view over the plane holds bases only)
                });
                if (mn <= mt[1]) mask[mt[2]] |= (uint32_t)mt[3];
            }
}

static void seed_stage(const pcp::Plan &p, Route route, const std::string &view, std::vector<uint32_t> &mask)
{
    if (p.nq == 0) { exhaustive(p, p.launches, route, view, mask); return; }
    const int n = (int)view.size();
    const int bm_off[3] = {0, (1 << 16) / 32, (1 << 16) / 32 + (1 << 14) / 32};
    for (int cl = 0; cl < p.nq; ++cl) {
        const int q = p.q[cl];
        for (int j = q - 1; j < n; ++j) {
            uint32_t idx = 0;
            bool bases = true;
            for (int t = 0; t < q; ++t) {
                const unsigned char b = (unsigned char)view[j - q + 1 + t];
                if (pcp::dna5(b) > 3) bases = false;
                if (route == Route::Bytes) idx = (idx << 2) | ((b >> 1) & 3u);       // the byte scan's code, first base highest
                else idx |= (uint32_t)pcp::dna5(b) << (2 * t);                       // the plane's code, first base lowest
            }
            if (!bases) continue;
            if (!((p.bitmaps[bm_off[cl] + (idx >> 5)] >> (idx & 31)) & 1u)) continue;
            const uint32_t e0 = p.first[p.first_off[cl] + idx], e1 = p.first[p.first_off[cl] + idx + 1];
            for (uint32_t e = e0; e < e1; ++e) {
                const int pi = p.entries[(size_t)e * 4], off = p.entries[(size_t)e * 4 + 1];
                const int32_t *mt = &p.piece_meta[(size_t)pi * 4];
                const int len = mt[0], k = mt[1];
                const int lo = std::max(0, j - q + 1 - off - k), hi = std::min(n, j - q + 1 - off + len + k);
                const uint32_t *eq = &p.piece_eq[(size_t)pi * 8];
                const int mn = best_score(view, lo, hi, len, [&](unsigned char b) { return eq[pcp::dna5(b)]; });
                if (mn <= k) mask[mt[2]] |= (uint32_t)mt[3];
            }
        }
    }
    exhaustive(p, p.rest_launches, route, view, mask);
}

// ---- structure ------------------------------------------------------------------------------------------------------------
typedef std::vector<uint32_t> PieceId;      // len, k, mask word, mask bit, Eq words of A, C, G, T
typedef std::map<PieceId, int> Pieces;      // a multiset: two pieces of one adapter may look the same

static Pieces slots_of(const pcp::Plan &p, const std::vector<pcp::Launch> &ls, Route route, int opt)
{
    const size_t rows = route == Route::PlaneTotal ? 4 : 256;
    Pieces got;
    for (const pcp::Launch &L : ls)
        for (int g = 0; g < L.groups; ++g)
            for (int slot = 0; slot < L.P; ++slot) {
                const int32_t *mt = &p.meta[L.meta_off + ((size_t)g * L.P + slot) * 4];
                const uint32_t *tab = &p.tables[L.table_off + (size_t)g * rows * L.P + slot];
                if (mt[0] == 0) {                                  // an idle slot: zero metadata, every row all ones
                    if (mt[1] | mt[2] | mt[3]) fail("idle slot with metadata", route, opt);
                    for (size_t r = 0; r < rows; ++r) if (tab[r * L.P] != 0xFFFFFFFFu) fail("idle slot with an Eq row", route, opt, (long)r);
                    continue;
                }
                PieceId id = {(uint32_t)mt[0], (uint32_t)mt[1], (uint32_t)mt[2], (uint32_t)mt[3]};
                for (char ch : std::string("ACGT")) id.push_back(tab[(rows == 4 ? (size_t)pcp::dna5((unsigned char)ch) : (size_t)(unsigned char)ch) * L.P]);
                ++got[id];
            }
    return got;
}

// the pieces the rules of the plan give, restated: <= 32 bases whole; longer with k <= 8 the first 32 bases; else ceil(m / 32)
// nearly equal pieces with floor(k / pieces) edits each
static Pieces expected_pieces(const std::vector<std::string> &adapters, const std::vector<int32_t> &ids, const std::vector<int32_t> &ks, Route route)
{
    Pieces want;
    for (size_t j = 0; j < ids.size(); ++j) {
        const std::string &ad = adapters[ids[j]];
        const int m = (int)ad.size(), k = ks[j] < 0 ? m : ks[j];
        if (m == 0) continue;
        std::vector<std::pair<int, int>> cuts;      // begin, len
        int kk = k;
        if (m > 32 && k <= 8) cuts.push_back({0, 32});
        else {
            const int np = (m + 31) / 32;
            kk = k / np;
            for (int t = 0, pos = 0; t < np; ++t) { const int len = m / np + (t < m % np ? 1 : 0); cuts.push_back({pos, len}); pos += len; }
        }
        for (auto &c : cuts) {
            PieceId id = {(uint32_t)c.second, (uint32_t)kk, (uint32_t)(j / 32), 1u << (j % 32)};
            for (int code = 0; code < 4; ++code) {
                uint32_t e = c.second >= 32 ? 0u : (0xFFFFFFFFu >> c.second);
                for (int r = 0; r < c.second; ++r) {
                    const int a = pcp::dna5((unsigned char)ad[c.first + r]);
                    if (a == code || (a == 4 && route == Route::PlaneTotal)) e |= 1u << (32 - c.second + r);
                }
                id.push_back(e);
            }
            ++want[id];
        }
    }
    return want;
}

static void check_structure(const pcp::Plan &p, const std::vector<std::string> &adapters, const std::vector<int32_t> &ids,
                            const std::vector<int32_t> &ks, Route route, int opt, const pcp::Options &o)
{
    const Pieces want = expected_pieces(adapters, ids, ks, route);
    if (slots_of(p, p.launches, route, opt) != want) fail("the launches over all pieces do not hold each piece once", route, opt);
    Pieces split = slots_of(p, p.nq > 0 ? p.rest_launches : p.launches, route, opt);
    long nrest = 0;
    for (auto &kv : split) nrest += kv.second;
    if (p.nq == 0 && p.npieces != 0) fail("seeded pieces without a seed length", route, opt);
    for (int i = 0; i < p.npieces; ++i) {
        PieceId id;
        for (int t = 0; t < 4; ++t) id.push_back((uint32_t)p.piece_meta[(size_t)i * 4 + t]);
        for (int t = 0; t < 4; ++t) id.push_back(p.piece_eq[(size_t)i * 8 + t]);
        ++split[id];
    }
    if (split != want) fail("seeded + rest is not each piece once", route, opt, p.npieces, nrest);
    if (p.seeds_only == (nrest > 0 || p.npieces == 0)) fail("the seeds-only flag", route, opt, p.npieces, nrest);
    if (o.no_seeds && p.nq != 0) fail("seeds under no_seeds", route, opt);
    if (p.nq > 0 && (p.q[0] > 8 || p.q[p.nq - 1] < 6)) fail("seed length", route, opt);
    for (int t = 1; t < p.nq; ++t) if (p.q[t] >= p.q[t - 1]) fail("seed lengths not descending", route, opt);
    if (!o.force_multi_q && o.force_single_q && p.nq > 1) fail("several seed lengths under force_single_q", route, opt);
    double rate = 0.0;
    for (int cl = 0; cl < p.nq; ++cl) {
        const uint32_t ngram = 1u << (2 * p.q[cl]);
        rate += (double)(p.first[p.first_off[cl] + ngram] - p.first[p.first_off[cl]]) / (double)ngram;
    }
    if (rate != p.rate) fail("rate", route, opt);
    n_seeded += p.npieces;
    n_rest += nrest;
}

// ---- cases ----------------------------------------------------------------------------------------------------------------
static std::string mutated(Rng &rng, std::string s, int edits)
{
    for (int e = 0; e < edits && !s.empty(); ++e) {
        const int at = rng.below((int)s.size());
        switch (rng.below(3)) {
            case 0: s[at] = rng.base(); break;
            case 1: s.insert(s.begin() + at, rng.base()); break;
            default: s.erase(s.begin() + at); break;
        }
    }
    return s;
}

static bool only_bases(const std::string &s)
{
    for (char ch : s) if (pcp::dna5((unsigned char)ch) > 3) return false;
    return true;
}

struct Case { std::vector<std::string> adapters, reads; std::vector<int32_t> ids, ks; };

static Case make_case(Rng &rng, long ci)
{
    // 1..13 adapters out of a panel a little larger, in any order: lengths 5..32, some 33..80, now and then none at all
    const int nad = (int)(ci % 13) + 1;
    const bool with_n = ci % 4 == 3;
    std::vector<std::string> adapters;
    for (int i = 0; i < nad + 2; ++i) {
        std::string ad = rng.seq(rng.chance(20) ? rng.in(33, 80) : rng.in(5, 32));
        if (rng.chance(2)) ad.clear();
        if (with_n && rng.chance(40))
            for (int t = rng.in(1, 2); t > 0 && !ad.empty(); --t) ad[rng.below((int)ad.size())] = "NnXacgu"[rng.below(7)];
        adapters.push_back(ad);
    }
    std::vector<int32_t> ids, ks;
    for (int i = 0; i < nad + 2; ++i) ids.push_back(i);
    std::shuffle(ids.begin(), ids.end(), rng.g);
    ids.resize(nad);
    const double thr = 70.0 + 0.5 * rng.below(61);                // 70 .. 100
    for (int j = 0; j < nad; ++j) {
        const int m = (int)adapters[ids[j]].size();
        const int pick = rng.below(10);
        ks.push_back(pick == 0 ? -1 : pick == 1 ? 0 : pcp::max_edits(m, rng.chance(70) ? thr : 70.0 + 0.5 * rng.below(61)));
    }
    // reads of 40..400 bases, copies of the adapters with 0..k + 2 edits planted in them
    std::vector<std::string> reads;
    for (int r = 0; r < 3; ++r) {
        std::string rd = rng.seq(rng.in(40, 400));
        for (int t = rng.below(3); t > 0; --t) {
            const int j = rng.below(nad);
            const std::string &ad = adapters[ids[j]];
            const int k = ks[j] < 0 ? (int)ad.size() : ks[j];
            const std::string copy = mutated(rng, ad, rng.in(0, std::min(k, 40) + 2));
            if (copy.size() > rd.size()) continue;
            rd.replace(rng.below((int)(rd.size() - copy.size()) + 1), copy.size(), copy);
        }
        if (with_n)
            for (int t = rng.below(4); t > 0; --t) rd[rng.below((int)rd.size())] = "NnX-acgtU"[rng.below(9)];
        reads.push_back(rd);
    }
    return Case{adapters, reads, ids, ks};
}

static void check_case(const Case &c, unsigned &remainders)
{
    const std::vector<std::string> &adapters = c.adapters, &reads = c.reads;
    const std::vector<int32_t> &ids = c.ids, &ks = c.ks;
    const int nad = (int)ids.size();
    std::vector<std::vector<int>> dist(reads.size(), std::vector<int>(nad, 0));
    for (size_t r = 0; r < reads.size(); ++r)
        for (int j = 0; j < nad; ++j) {
            const std::string &ad = adapters[ids[j]];
            dist[r][j] = pc_oracle_min_edits(reads[r].data(), (int)reads[r].size(), ad.data(), (int)ad.size());
        }

    const int words = (nad + 31) / 32;
    for (Route route : {Route::Bytes, Route::PlaneSeeds, Route::PlaneTotal})
        for (int opt = 0; opt < 4; ++opt) {
            pcp::Options o;
            o.no_seeds = opt == 1; o.force_multi_q = opt == 2; o.force_single_q = opt == 3;
            pcp::Plan p;
            if (pcp::build(adapters, ids.data(), ks.data(), nad, route, o, p)) { fail("build refused the list", route, opt); continue; }
            check_structure(p, adapters, ids, ks, route, opt, o);
            if (route == Route::Bytes && opt == 0) {
                long np = 0;
                for (const pcp::Launch &L : p.launches)
                    for (int s = 0; s < L.groups * L.P; ++s) np += p.meta[L.meta_off + (size_t)s * 4] != 0;
                remainders |= 1u << (np % 8);
            }
            for (size_t r = 0; r < reads.size(); ++r) {
                const std::string view = view_of(reads[r], route);
                std::vector<uint32_t> all(words, 0u), staged(words, 0u);
                exhaustive(p, p.launches, route, view, all);
                seed_stage(p, route, view, staged);
                if (all != staged) fail("the seed stage's mask differs from the exhaustive one", route, opt, (long)r);
                // (a list the seeds-only route refuses gets no mask from it: its byte tables are never launched over the plane)
                if (route == Route::PlaneSeeds && !p.seeds_only && !p.launches.empty()) continue;
                for (int j = 0; j < nad; ++j) {
                    const std::string &ad = adapters[ids[j]];
                    const int m = (int)ad.size(), k = ks[j] < 0 ? m : ks[j];
                    const bool got = (all[j / 32] >> (j % 32)) & 1u, want = dist[r][j] <= k;
                    if (m == 0) { if (got) fail("an empty adapter's bit is set", route, opt, (long)r, j); continue; }
                    const bool exact = m <= 32 && (route == Route::Bytes || (only_bases(ad) && only_bases(reads[r])));
                    if (exact ? got != want : (want && !got)) fail(exact ? "mask is not the oracle's" : "a pair within the bound was dropped", route, opt, (long)r, j);
                    if (m > 32 && want) ++n_long;
                }
            }
        }
}

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 600;
    if (argc > 2) g_seed = strtoull(argv[2], nullptr, 10);
    Rng rng(g_seed);
    unsigned remainders = 0;
    for (g_case = 0; g_case < cases; ++g_case) check_case(make_case(rng, g_case), remainders);
    if (cases >= 200 && remainders != 0xFFu) fail("a remainder of the group split never occurred", Route::Bytes, 0, (long)remainders);
    printf("bad=%ld cases=%ld seeded=%ld rest=%ld long=%ld seed=%llu\n", bad, cases, n_seeded, n_rest, n_long, g_seed);
    return bad ? 1 : 0;
}
