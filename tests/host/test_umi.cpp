// Host-side test of porechop_amd/csrc/pc_umi.h -- the read columns under an adapter's degenerate rows -- over paths that
// pcpath::align_path_sets (pc_paths.h) produces on the host, as tests/host/test_paths.cpp obtains them: the same routine and
// the same nibble packing the device runs per lane.
//
// Per case: an adapter of 1..128 rows with its degenerate rows at row 0, at the last row, in a single row, over the whole
// adapter or in two blocks with fixed rows between; an instance of it planted in a window of 0..150 bases whole, clipped by
// either window edge inside or outside the span, with a substitution, an insertion or a deletion inside the span or at one
// of its edges, or not at all; one of three schemes (the default, a linear one, one the packed kernels refuse).
//   (a) pcu::span against a naive scan of the letters;
//   (b) pcu::extract against a naive forward replay: the operations expanded to a list, the columns marked one by one,
//       the marks checked to be one run;
//   (c) pcu::qualifies, with the rounding of pc_record.h restated for the host, against the torch expression of phase B
//       evaluated in C with the oracle's identities (the reference's "%f", printed and parsed back).
//
//   g++ -O2 -std=c++17 -fsanitize=address,undefined -I porechop_amd/csrc tests/host/test_umi.cpp && ./a.out [cases [seed]]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pc_paths.h"
#include "pc_slow.h"
#include "pc_umi.h"

static int dna5(unsigned char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

struct Mem {
    std::vector<int> *m, *h; std::vector<uint32_t> *t; int groups;
    int &M(int i) { return (*m)[i]; }
    int &H(int i) { return (*h)[i]; }
    void put(int j, int g, uint32_t w) { (*t).at((size_t)j * groups + g) = w; }
    uint32_t get(int j, int g) { return (*t).at((size_t)j * groups + g); }
};

struct Rec { int rs, re, matches, aligned_len; };
struct Rule { int end_size, min_trim_size, extra_end_trim; double end_threshold; };

// the identity Python sees: "%f" printed by the reference and parsed back
static double oracle_identity(int matches, int len)
{
    if (len == 0) return NAN;
    char buf[64];
    snprintf(buf, sizeof buf, "%f", 100.0 * (double)matches / (double)len);
    return strtod(buf, nullptr);
}
// pc_record.h's identity(), restated for the host (the header is device code)
static double record_identity(int matches, int len)
{
    const double x = (100.0 * (double)matches) / (double)len;
    return rint(x * 1e6) / 1e6;
}

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 20000;
    std::mt19937_64 rng(argc > 2 ? atol(argv[2]) : 20240611);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    const int schemes[3][4] = {{3, -6, -5, -2}, {3, -6, -5, -5}, {300, -600, -500, -200}};
    const char *degenerate = "RYSWKMBDHVN";
    long done = 0, bad = 0, status_n[4] = {0, 0, 0, 0}, len0 = 0, len_above = 0, len_below = 0, qual_yes = 0, qual_no = 0,
         placement_n[5] = {0, 0, 0, 0, 0}, plant_n[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gapped_in_span = 0;
    while (done < cases) {
        const int *sc = schemes[done % 3];
        const int m = pick(0, 9) < 3 ? pick(1, 12) : pick(1, 128);
        // ---- the adapter: where its degenerate rows are ----
        const int placement = pick(0, 4);
        std::vector<char> deg(m, 0);
        if (placement == 0) { const int k = pick(1, m); for (int r = 0; r < k; ++r) deg[r] = 1; }                 // from row 0
        else if (placement == 1) { const int k = pick(1, m); for (int r = m - k; r < m; ++r) deg[r] = 1; }       // to the last row
        else if (placement == 2) deg[pick(0, m - 1)] = 1;                                                        // a single row
        else if (placement == 3) for (int r = 0; r < m; ++r) deg[r] = 1;                                         // the whole adapter
        else {                                                                                                   // two blocks
            const int a = pick(0, m - 1), b = pick(a, m - 1);
            const int a1 = pick(a, b), b0 = pick(a1, b);
            for (int r = a; r <= a1; ++r) deg[r] = 1;
            for (int r = b0; r <= b; ++r) deg[r] = 1;
        }
        std::string ad(m, 'A');
        for (int r = 0; r < m; ++r) ad[r] = deg[r] ? degenerate[pick(0, 10)] : "ACGT"[pick(0, 3)];
        std::vector<uint32_t> sets(m);
        for (int r = 0; r < m; ++r) sets[r] = pcl::letter_set((uint8_t)ad[r], true);
        // (a) the span
        int want0 = -1, want1 = -1;
        for (int r = 0; r < m; ++r) if (deg[r]) { if (want0 < 0) want0 = r; want1 = r; }
        int u0 = -7, u1 = -7;
        const bool has = pcu::span([&](int k) { return sets[k]; }, m, &u0, &u1);
        const char *why = nullptr;
        if (!has || u0 != want0 || u1 != want1) why = "(a) span";
        {
            int f0, f1;
            std::string fixed(m, 'A');
            for (int r = 0; r < m; ++r) fixed[r] = "ACGTU"[pick(0, 4)];
            if (pcu::span([&](int k) { return pcl::letter_set((uint8_t)fixed[k], true); }, m, &f0, &f1) || f0 != -1 || f1 != -1) why = "(a) span of a fixed adapter";
            if (pcu::span([&](int k) { return pcl::letter_set((uint8_t)ad[k], false); }, m, &f0, &f1)) why = "(a) span with wildcards off";
        }
        // ---- an instance of the adapter, edited ----
        std::string inst(m, 'A');
        for (int r = 0; r < m; ++r) {
            std::string members;
            for (int k = 0; k < 4; ++k) if (sets[r] >> k & 1) members += "ACGT"[k];
            inst[r] = members[pick(0, (int)members.size() - 1)];
        }
        const int plant = pick(0, 7);       // 0 whole, 1 clipped left, 2 clipped right, 3 substitution, 4 insertion, 5 deletion, 6 absent, 7 several edits
        auto edit_row = [&]() {
            const int w = pick(0, 5);       // inside the span, at its edges, just outside them
            int r = w == 0 ? pick(u0, u1) : w == 1 ? u0 : w == 2 ? u1 : w == 3 ? u0 - 1 : w == 4 ? u1 + 1 : pick(0, m - 1);
            return r < 0 ? 0 : r >= m ? m - 1 : r;
        };
        std::string body = inst;
        int cut_left = 0, cut_right = 0;
        auto one_edit = [&](int kind) {
            if (body.empty()) return;
            int r = edit_row();
            if (r >= (int)body.size()) r = (int)body.size() - 1;
            if (kind == 3) { char c; do c = "ACGT"[pick(0, 3)]; while (c == body[r]); body[r] = c; }
            else if (kind == 4) body.insert(body.begin() + r, "ACGT"[pick(0, 3)]);
            else body.erase(body.begin() + r);
        };
        if (plant == 1) { const int w = pick(0, 2); cut_left = w == 0 ? pick(u0, u1) + pick(0, 1) : w == 1 ? pick(0, u0) : pick(0, m); if (cut_left > m) cut_left = m; }
        else if (plant == 2) { const int w = pick(0, 2); const int keep = w == 0 ? pick(u0, u1) + pick(0, 1) : w == 1 ? pick(u1 + 1, m) : pick(0, m); cut_right = m - (keep > m ? m : keep); }
        else if (plant >= 3 && plant <= 5) one_edit(plant);
        else if (plant == 7) for (int k = pick(2, 4); k > 0; --k) one_edit(pick(3, 5));
        std::string rd;
        auto noise = [&](int k) { std::string s(k, 'A'); for (char &c : s) c = "ACGTACGTACGTN"[pick(0, 12)]; return s; };
        if (plant == 6) rd = noise(pick(0, 9) == 0 ? 0 : pick(0, 150));
        else if (plant == 1) { rd = body.substr((size_t)cut_left); rd += noise(pick(0, 20)); }                    // the window starts inside the instance
        else if (plant == 2) { rd = noise(pick(0, 20)); rd += body.substr(0, body.size() - (size_t)cut_right); }  // the window ends inside it
        else { rd = noise(pick(0, 25)); rd += body; rd += noise(pick(0, 25)); }
        if (rd.size() > 150) {              // a long adapter: the window's edge clips it, at either end
            if (pick(0, 1)) rd = rd.substr(0, 150); else rd = rd.substr(rd.size() - 150);
        }
        if (pick(0, 40) == 0 && rd.size() < 150) rd = noise(150 - (int)rd.size()) + rd;                            // a full window, flush cases
        const int n = (int)rd.size();
        if (!pcs::fits(n, m, sc[0], sc[1], sc[2], sc[3])) continue;
        ++done;
        ++placement_n[placement]; ++plant_n[plant];
        // ---- the path ----
        const int groups = pcpath::row_groups(m);
        std::vector<int> M(m + 1), H(m + 1);
        std::vector<uint32_t> T((size_t)(n + 1) * groups, 0xffffffffu);
        const int64_t words = pcpath::ops_words(n, m);
        std::vector<uint32_t> ops((size_t)words + 1, 0xdeadbeefu);
        pcw::Digest d;
        int32_t head[4] = {-1, -1, -1, -1};
        int sink_bad = 0;
        const int err = pcpath::align_path_sets(n, m, [&](int k) { return dna5((unsigned char)rd[k]); }, [&](int k) { return sets[k]; }, sc[0], sc[1],
                                                sc[2], sc[3], Mem{&M, &H, &T, groups}, d, head,
                                                [&](int k, uint32_t w) { if (k < 0 || k >= words) sink_bad = 1; else ops[k] = w; });
        if (err || sink_bad) why = "path routine";
        const int L = head[0];
        // (b) pcu::extract, reading only the words the path wrote, last word first, each once
        int reads_bad = 0, last_word = (L + 15) / 16;
        const pcu::Umi got = pcu::extract(head, [&](int k) {
            if (k != last_word - 1 || k < 0) reads_bad = 1;
            last_word = k;
            return ops.at((size_t)k);
        }, u0, u1);
        if (reads_bad || (L > 0 && last_word != 0)) why = why ? why : "(b) order of the word reads";
        std::vector<char> fwd((size_t)L);
        for (int k = 0; k < L; ++k) fwd[(size_t)(L - 1 - k)] = "=XID"[(ops[(size_t)k / 16] >> (2 * (k % 16))) & 3u];
        std::vector<char> mark((size_t)n + 1, 0);
        int i = head[1], j = head[2], covered = 0, last_row = -1, gaps_inside = 0;
        for (int k = 0; k < L && !why; ++k) {
            const char op = fwd[(size_t)k];
            if (op == '=' || op == 'X') {
                if (i >= n || j >= m) { why = "(b) replay left the rectangle"; break; }
                if (j >= u0 && j <= u1) { mark[(size_t)i] = 1; ++covered; }
                last_row = j; ++i; ++j;
            } else if (op == 'I') {
                if (i >= n) { why = "(b) replay left the rectangle"; break; }
                if (j > u0 && j <= u1) { mark[(size_t)i] = 1; ++gaps_inside; }
                ++i;
            } else {
                if (j >= m) { why = "(b) replay left the rectangle"; break; }
                if (j >= u0 && j <= u1) ++gaps_inside;
                last_row = j; ++j;
            }
        }
        int first = -1, len = 0, runs = 0;
        for (int c = 0; c < n; ++c) if (mark[(size_t)c]) { if (len == 0) first = c; ++len; if (c == 0 || !mark[(size_t)c - 1]) ++runs; }
        const int complete = (head[2] <= u0 && last_row >= u1) ? 1 : 0;
        if (!why && runs > 1) why = "(b) the marked columns are not one run";
        if (!why && (got.first != first || got.len != len || got.covered != covered || got.complete != complete)) why = "(b) extract != replay";
        if (!why && len == 0 && got.first != -1) why = "(b) empty run";
        // (c) the rule
        const int side = pick(0, 1);
        const Rule rule = {150, pick(0, 3) ? 4 : pick(1, 40), 2, pick(0, 3) ? 75.0 : (double)pick(0, 100)};
        const Rec rec = {d.read_start, d.read_end, d.matches, d.aligned_len};
        const bool q = pcu::qualifies(rec, side, rule, record_identity);
        {
            const bool ok = rec.rs != -1 && rec.rs >= 0;
            const double partial = oracle_identity(rec.matches, rec.aligned_len);
            const int rs = rec.rs, re = rec.re + 1;
            const bool cond = side == 0 ? ok && (partial > rule.end_threshold) && (re != rule.end_size) && ((re - rs) >= rule.min_trim_size)
                                        : ok && (partial > rule.end_threshold) && (rs != 0) && ((re - rs) >= rule.min_trim_size);
            if (!why && q != cond) why = "(c) qualifies != phase B's condition";
        }
        const int status = rec.rs < 0 ? 1 : !q ? 2 : got.complete ? 0 : 3;
        if (!why && n == 0 && status != 1) why = "empty window";
        ++status_n[status];
        qual_yes += q; qual_no += !q && rec.rs >= 0;
        if (rec.rs >= 0) {
            len0 += got.len == 0; len_above += got.len > u1 - u0 + 1; len_below += got.len < u1 - u0 + 1 && got.len > 0;
            gapped_in_span += gaps_inside > 0;
        }
        if (why && ++bad <= 10)
            printf("MISMATCH %s rd=%s ad=%s scores=%d,%d,%d,%d span=%d..%d head=%d,%d,%d,%d got=%d,%d,%d,%d want=%d,%d,%d,%d\n", why, rd.c_str(),
                   ad.c_str(), sc[0], sc[1], sc[2], sc[3], u0, u1, head[0], head[1], head[2], head[3], got.first, got.len, got.covered,
                   got.complete, first, len, covered, complete);
    }
    printf("cases=%ld bad=%ld status0=%ld status1=%ld status2=%ld status3=%ld len0=%ld len_above=%ld len_below=%ld qualifies=%ld not=%ld gapped_in_span=%ld "
           "row0=%ld lastrow=%ld single=%ld whole=%ld blocks=%ld plant_whole=%ld clip_left=%ld clip_right=%ld sub=%ld ins=%ld del=%ld absent=%ld several=%ld\n",
           done, bad, status_n[0], status_n[1], status_n[2], status_n[3], len0, len_above, len_below, qual_yes, qual_no, gapped_in_span,
           placement_n[0], placement_n[1], placement_n[2], placement_n[3], placement_n[4], plant_n[0], plant_n[1], plant_n[2], plant_n[3],
           plant_n[4], plant_n[5], plant_n[6], plant_n[7]);
    return bad ? 1 : 0;
}
