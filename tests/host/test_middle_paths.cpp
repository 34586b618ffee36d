// Host-side test of porechop_amd/csrc/pc_middle_paths.h -- the path of a middle hit from a bounded window of the masked
// read -- against pcpath::align_path (pc_paths.h) over the WHOLE, explicitly masked read, with the device's nibble packing
// (eight rows to a dword) as the memory policy of both.
//
// Per case: a read, an adapter, a scheme and 0..4 masked runs.  The reference run gives record, head and operations; its
// read_end + 1 is the `re` a hit list would carry.  The windowed run gets re, the UNMASKED read and the runs as intervals
// (W and window from pcb::compute_bounds for the adapter's length, the whole read where it refuses).  Record, head and every
// operation must be equal; the windowed run may ask for no read base outside [c0, c1) and no trace column outside the window.
//
// Cases: (1) seeded random reads with mutated copies, adapters of 1, 7, 8, 9, 17, 28, 33, 68 and 111 bases, over bounded
// affine, open-above-extend and linear schemes and one scheme compute_bounds refuses; (2) the reads of a case file, one
// "read adapter match mismatch gap_open gap_extend" per line (tests/test_middle_paths_host.py writes the gap-stretched copies
// of tests/stretchgen.py there, so that paths as wide as W and warm-ups as long as SPAN occur).  The masked runs are
// placed around the window of the unmasked alignment: astride c0, astride c1, next to the hit, inside the window, anywhere.
//
//   g++ -O2 -std=c++17 -I porechop_amd/csrc tests/host/test_middle_paths.cpp
//   ./a.out [random cases [seed [case file]]]
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "pc_bounds.h"
#include "pc_middle_paths.h"

static int dna5(unsigned char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

struct Mem {
    std::vector<int> *m, *h; std::vector<uint32_t> *t; int groups, cols;
    int &M(int i) { return (*m).at(i); }
    int &H(int i) { return (*h).at(i); }
    // column j = 1 .. cols only: .at() and the sanitizers see anything else
    void put(int j, int g, uint32_t w) { if (j < 1 || j > cols) abort(); (*t).at((size_t)j * groups + g) = w; }
    uint32_t get(int j, int g) { if (j < 1 || j > cols) abort(); return (*t).at((size_t)j * groups + g); }
};

struct Result { pcw::Digest d; int32_t head[4]; std::vector<uint32_t> ops; int err; };

static bool same(const Result &a, const Result &b)
{
    if (memcmp(&a.d, &b.d, sizeof a.d) || memcmp(a.head, b.head, sizeof a.head) || a.err != b.err) return false;
    for (int k = 0; k < a.head[0]; ++k)
        if (((a.ops.at(k / 16) >> (2 * (k % 16))) & 3u) != ((b.ops.at(k / 16) >> (2 * (k % 16))) & 3u)) return false;
    return true;
}

struct Counts {
    long cases = 0, bad = 0, skipped = 0, interior = 0, c0_zero = 0, cut_by_end = 0, mask_inside = 0, mask_astride_c0 = 0,
         mask_astride_c1 = 0, mask_adjacent = 0, near_W = 0, linear = 0, refused = 0, open_above = 0, warm_full = 0, widest_path = 0;
    long rows[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
static const int kRows[9] = {1, 7, 8, 9, 17, 28, 33, 68, 111};

typedef std::vector<std::pair<int, int>> Runs;

static Result whole(const std::string &masked, const std::string &ad, const int sc[4])
{
    const int n = (int)masked.size(), m = (int)ad.size(), groups = pcpath::row_groups(m);
    std::vector<int> M(m + 1), H(m + 1);
    std::vector<uint32_t> T((size_t)(n + 1) * std::max(1, groups), 0xffffffffu);
    Result r;
    r.ops.assign((size_t)pcpath::ops_words(n, m) + 1, 0u);
    r.err = pcpath::align_path(n, m, [&](int k) { return dna5((unsigned char)masked[k]); }, [&](int k) { return dna5((unsigned char)ad[k]); },
                               sc[0], sc[1], sc[2], sc[3], Mem{&M, &H, &T, groups, n}, r.d, r.head,
                               [&](int k, uint32_t w) { r.ops.at(k) = w; });
    return r;
}

static void window_of(int n, int m, int re, const int sc[4], int &c0, int &c1, pcb::Bounds &b, bool &bounded)
{
    bounded = pcb::compute_bounds(sc[0], sc[1], sc[2], sc[3], m, b);
    if (!bounded) b = {0, 0, 0};
    pcpath::hit_window(n, re, bounded, b.W, b.window, c0, c1);
}

static Result windowed(const std::string &read, const Runs &runs, const std::string &ad, const int sc[4], int re, int &outside)
{
    const int n = (int)read.size(), m = (int)ad.size(), groups = pcpath::row_groups(m);
    int c0, c1;
    pcb::Bounds b;
    bool bounded;
    window_of(n, m, re, sc, c0, c1, b, bounded);
    const int nc = c1 - c0;
    std::vector<int> M(m + 1), H(m + 1);
    std::vector<uint32_t> T((size_t)(nc + 1) * std::max(1, groups), 0xffffffffu);
    Result r;
    r.ops.assign((size_t)pcpath::ops_words(nc, m) + 1, 0u);
    r.err = pcpath::align_path_window(
        n, m, c0, c1,
        [&](int k) {
            if (k < c0 || k >= c1) { ++outside; return 4; }
            int code = dna5((unsigned char)read[k]);
            for (const auto &iv : runs) if (k >= iv.first && k < iv.second) code = 4;
            return code;
        },
        [&](int k) { return dna5((unsigned char)ad[k]); }, sc[0], sc[1], sc[2], sc[3], Mem{&M, &H, &T, groups, nc}, r.d, r.head,
        [&](int k, uint32_t w) { r.ops.at(k) = w; });
    return r;
}

static std::string mask(const std::string &read, const Runs &runs)
{
    std::string s = read;
    for (const auto &iv : runs) for (int k = std::max(0, iv.first); k < std::min((int)s.size(), iv.second); ++k) s[k] = '-';
    return s;
}

template <typename Pick>
static void one_case(const std::string &read, const std::string &ad, const int sc[4], int nruns, Pick pick, Counts &cnt)
{
    const int n = (int)read.size(), m = (int)ad.size();
    // where the unmasked alignment's window lies: the runs are placed around it
    Result plain = whole(read, ad, sc);
    Runs runs;
    if (!plain.err && plain.d.read_start >= 0 && plain.d.score > 0) {
        int c0, c1;
        pcb::Bounds b;
        bool bounded;
        const int rs = plain.d.read_start, re = plain.d.read_end + 1;
        window_of(n, m, re, sc, c0, c1, b, bounded);
        for (int k = 0; k < nruns; ++k) {
            const int len = pick(1, 40), kind = pick(0, 5);
            int s;
            if (kind == 0) s = c0 - pick(1, len);                       // astride c0 (or before the read when c0 == 0)
            else if (kind == 1) s = c1 - pick(0, len);                  // astride or up to c1
            else if (kind == 2) s = rs - len;                           // ends where the hit starts
            else if (kind == 3) s = re;                                 // starts where the hit ends
            else if (kind == 4) s = c0 + pick(0, std::max(0, rs - c0 - len));   // inside the window, left of the hit
            else s = pick(0, std::max(0, n - len));
            int e = s + len;
            s = std::max(0, s); e = std::min(n, e);
            if (e > s && (e <= rs || s >= re || kind == 5)) runs.push_back({s, e});
        }
    }
    const std::string masked = mask(read, runs);
    const Result ref = whole(masked, ad, sc);
    if (ref.err || ref.d.read_start < 0 || ref.d.score <= 0) { ++cnt.skipped; return; }     // no alignment a hit list could carry
    const int rs = ref.d.read_start, re = ref.d.read_end + 1;
    int c0, c1, outside = 0;
    pcb::Bounds b;
    bool bounded;
    window_of(n, m, re, sc, c0, c1, b, bounded);
    const Result win = windowed(read, runs, ad, sc, re, outside);
    ++cnt.cases;
    long read_steps = 0, adapter_steps = 0;
    for (int k = 0; k < ref.head[0]; ++k) {
        const uint32_t op = (ref.ops[k / 16] >> (2 * (k % 16))) & 3u;
        read_steps += op != pcpath::OP_D; adapter_steps += op != pcpath::OP_I;
    }
    const long I = ref.head[2] + adapter_steps;              // the end cell's row
    const bool ok = same(ref, win) && outside == 0;
    if (!ok && ++cnt.bad <= 10) {
        printf("MISMATCH n=%d m=%d scores=%d,%d,%d,%d re=%d window [%d,%d) runs=%zu outside=%d\n ref %d,%d,%d,%d,%d m=%d al=%d fl=%d head=%d,%d,%d,%d err=%d\n win %d,%d,%d,%d,%d m=%d al=%d fl=%d head=%d,%d,%d,%d err=%d\n rd=%s\n ad=%s\n",
               n, m, sc[0], sc[1], sc[2], sc[3], re, c0, c1, runs.size(), outside, ref.d.read_start, ref.d.read_end, ref.d.adapter_start,
               ref.d.adapter_end, ref.d.score, ref.d.matches, ref.d.aligned_len, ref.d.full_len, ref.head[0], ref.head[1], ref.head[2],
               ref.head[3], ref.err, win.d.read_start, win.d.read_end, win.d.adapter_start, win.d.adapter_end, win.d.score, win.d.matches,
               win.d.aligned_len, win.d.full_len, win.head[0], win.head[1], win.head[2], win.head[3], win.err, masked.c_str(), ad.c_str());
    }
    cnt.linear += sc[2] == sc[3]; cnt.open_above += sc[2] > sc[3]; cnt.refused += !bounded;
    for (int q = 0; q < 9; ++q) cnt.rows[q] += m == kRows[q];
    if (bounded) {
        cnt.interior += c0 > 0 && c1 < n;
        cnt.c0_zero += c0 == 0;
        cnt.cut_by_end += c1 == n && I < m;
        cnt.near_W += m >= 17 && b.W - read_steps <= 2;           // (short adapters: W - m <= 2 says nothing)
        cnt.warm_full += c0 > 0;                                   // a warm-up of the full window - W columns
        cnt.widest_path = std::max(cnt.widest_path, read_steps);
        bool inside = false, a0 = false, a1 = false, adj = false;
        for (const auto &iv : runs) {
            inside |= iv.first >= c0 && iv.second <= c1;
            a0 |= c0 > 0 && iv.first < c0 && iv.second > c0;
            a1 |= c1 < n && iv.first < c1 && iv.second > c1;
            adj |= iv.second == rs || iv.first == re;
        }
        cnt.mask_inside += inside; cnt.mask_astride_c0 += a0; cnt.mask_astride_c1 += a1; cnt.mask_adjacent += adj;
    }
}

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? atol(argv[2]) : 12345);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    Counts cnt;
    // bounded affine, open above extend, linear, no-drift, and one compute_bounds refuses (match * m above its limit)
    static const int SCHEMES[][4] = {{3, -6, -5, -2}, {3, -6, -2, -5}, {5, -4, -10, -1}, {3, -6, -5, -5}, {1, -1, -1, -1},
                                     {4, -7, -10, -140}, {20, -30, -25, -12}, {9000, -6, -5, -2}};
    const int nschemes = (int)(sizeof SCHEMES / sizeof SCHEMES[0]);
    for (long done = 0; done < cases; ++done) {
        const int *sc = SCHEMES[pick(0, nschemes - 1)];
        const int m = kRows[pick(0, 8)];
        std::string ad(m, 'A');
        for (char &c : ad) c = "ACGT"[pick(0, 3)];
        pcb::Bounds b;
        const bool bounded = pcb::compute_bounds(sc[0], sc[1], sc[2], sc[3], m, b);
        // reads around the window's size: shorter than it, a little longer, several times longer
        const int unit = bounded ? b.window + b.W : 300;
        const int shape = pick(0, 3);
        const int n = shape == 0 ? pick(1, std::max(1, unit / 2)) : shape == 1 ? pick(unit / 2, unit + 40) : pick(unit, std::min(3000, 3 * unit + 100));
        std::string rd(n, 'A');
        for (char &c : rd) c = "ACGT"[pick(0, 3)];
        // one or two mutated copies (substitutions, deleted and inserted bases), one of them possibly cut by an end of the read
        const int copies = pick(1, 2);
        for (int q = 0; q < copies; ++q) {
            std::string copy;
            for (int k = 0; k < m; ++k) {
                const int r = pick(0, 99);
                if (r < 6) copy += "ACGT"[pick(0, 3)];
                else if (r < 9) continue;
                else if (r < 12) { copy += ad[k]; copy += "ACGT"[pick(0, 3)]; }
                else copy += ad[k];
            }
            const int where = pick(0, 9);
            int s = where == 0 ? -pick(0, m / 2) : where == 1 ? n - (int)copy.size() + pick(0, m / 2) : pick(0, std::max(0, n - (int)copy.size()));
            for (int k = 0; k < (int)copy.size(); ++k) if (s + k >= 0 && s + k < n) rd[s + k] = copy[k];
        }
        one_case(rd, ad, sc, pick(0, 4), pick, cnt);
    }
    long from_file = 0;
    if (argc > 3) {
        std::ifstream in(argv[3]);
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string rd, ad;
            int sc[4];
            if (!(ss >> rd >> ad >> sc[0] >> sc[1] >> sc[2] >> sc[3])) continue;
            // each read once as it is and once with masked runs around its window
            one_case(rd, ad, sc, 0, pick, cnt);
            one_case(rd, ad, sc, pick(1, 4), pick, cnt);
            ++from_file;
        }
    }
    printf("cases=%ld bad=%ld skipped=%ld from_file=%ld interior=%ld c0_zero=%ld cut_by_end=%ld mask_inside=%ld mask_astride_c0=%ld "
           "mask_astride_c1=%ld mask_adjacent=%ld near_W=%ld warm_full=%ld linear=%ld open_above_extend=%ld refused=%ld widest_path=%ld",
           cnt.cases, cnt.bad, cnt.skipped, from_file, cnt.interior, cnt.c0_zero, cnt.cut_by_end, cnt.mask_inside, cnt.mask_astride_c0,
           cnt.mask_astride_c1, cnt.mask_adjacent, cnt.near_W, cnt.warm_full, cnt.linear, cnt.open_above, cnt.refused, cnt.widest_path);
    for (int q = 0; q < 9; ++q) printf(" rows%d=%ld", kRows[q], cnt.rows[q]);
    printf("\n");
    return cnt.bad ? 1 : 0;
}
