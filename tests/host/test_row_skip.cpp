// test_row_skip.cpp -- the row-skip proposition of pc_bounds.h (row_skip_plan) held, cell for cell, against the plain
// recurrence of pc_cell.h.  Host only.
//
// Two streams share a window of lower rows, as the two halves of a tile do: the longer adapter fills the R register rows,
// the shorter one sits bottom-aligned under its padding rows.  The skipping recurrence computes rows <= r0 in every
// column and rows > r0 only in the columns j'' .. j'' + W_low behind a column with M(r0, j'') >= theta in either stream;
// where the rows below are switched on their values of the column before are -infinity.  Checked, for every even r0
// row_skip_plan accepts (the rule's own r0 among them), for floors of 75 / 85 / 90 % identity:
//   claim 1   M^ <= M in every cell (a cell that is not computed counts as -infinity)
//   claim 2   every candidate end cell (last row, last column) with M >= F has M^ = M
//   (and once per pair at the floor of 100 %, F = match * m, on exact copies: there W_low = R - r0 and every column of it is used)
//   claim 3   a path that starts in column 0 below row r0 scores at most match * (R - r0 - 1) < F
//   and the consequences: the scout picks the same end cell whenever the true best is >= F; a pair below F stays below.
//   usage: test_row_skip [windows per case]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pc_bounds.h"
#include "pc_cell.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
int rnd_below(int n) { return n > 0 ? (int)(rnd() % (uint32_t)n) : 0; }

struct Scheme { int match, mismatch, open, ext; };

// M of every cell, rows 0..m, columns 0..n; on[j] says whether rows > i0 are computed in column j (i0 >= m: all of them).
// A cell that is not computed holds -infinity in all three states.
struct Matrix { int n, m; std::vector<int> M; int at(int i, int j) const { return M[(size_t)j * (m + 1) + i]; } };

Matrix run(const std::string &read, const std::string &ad, const Scheme &s, int i0, const std::vector<char> *on, bool only_below)
{
    const int n = (int)read.size(), m = (int)ad.size();
    Matrix x{n, m, std::vector<int>((size_t)(n + 1) * (m + 1), pcc::NEG_INF)};
    std::vector<int> Mc(m + 1, 0), Hc(m + 1, pcc::NEG_INF);          // the column state: M = 0 in column 0, H = -inf
    auto off = [&](int i, int j) { return (on && i > i0 && !(*on)[j]) || (only_below && i <= i0); };
    for (int i = 0; i <= m; ++i) {
        if (only_below && i <= i0) Mc[i] = pcc::NEG_INF;             // claim 3's matrix: no start at or above row i0
        x.M[i] = Mc[i];
    }
    // (column 0 of the skipping recurrence is what the kernel starts from: M = 0 in every row)
    for (int j = 1; j <= n; ++j) {
        int diag = only_below ? pcc::NEG_INF : 0, upM = only_below ? pcc::NEG_INF : 0, upV = pcc::NEG_INF;
        const int h = pcc::dna5_code((uint8_t)read[j - 1]);
        x.M[(size_t)j * (m + 1)] = upM;
        for (int i = 1; i <= m; ++i) {
            const int Mi = Mc[i];
            if (off(i, j)) {
                diag = Mi; Mc[i] = pcc::NEG_INF; Hc[i] = pcc::NEG_INF; upM = pcc::NEG_INF; upV = pcc::NEG_INF;
                continue;
            }
            const int sub = (h == pcc::dna5_code((uint8_t)ad[i - 1])) ? s.match : s.mismatch;
            // (-infinity is INT_MIN / 2: one more step down stays far below every real value and never overflows here)
            pcc::Cell c = pcc::cell(false, std::max(diag, pcc::NEG_INF / 2), sub, std::max(upM, pcc::NEG_INF / 2),
                                    std::max(upV, pcc::NEG_INF / 2), std::max(Mi, pcc::NEG_INF / 2), Hc[i], s.open, s.ext);
            Hc[i] = std::max(Hc[i], pcc::NEG_INF / 2);
            if (c.S < pcc::NEG_INF / 4) { c.S = pcc::NEG_INF; c.Vs = pcc::NEG_INF; }
            diag = Mi; Mc[i] = c.S; upM = c.S; upV = c.Vs;
            x.M[(size_t)j * (m + 1) + i] = c.S;
        }
    }
    return x;
}

// the scout over the candidate cells, in visiting order
void scout(const Matrix &x, int &best, int &I, int &J)
{
    best = 0; I = x.m; J = 0;
    for (int j = 1; j <= x.n; ++j)
        for (int i = 1; i <= x.m; ++i)
            if ((j == x.n || i == x.m) && x.at(i, j) > best) { best = x.at(i, j); I = i; J = j; }
}

std::string random_bases(int n) { std::string r(n, 'A'); for (char &c : r) c = "ACGT"[rnd_below(4)]; return r; }

// a read of n bases with mutated copies of the adapters planted: whole, cut by either edge, overlapping, absent
std::string make_read(int n, const std::string &a, const std::string &b)
{
    std::string r = random_bases(n);
    const int copies = rnd_below(4);
    for (int k = 0; k < copies && n > 0; ++k) {
        std::string c = (rnd() & 1) ? a : b;
        const int ident = 60 + rnd_below(41);
        std::string mut;
        for (char ch : c) {
            const int u = rnd_below(100);
            if (u < ident) mut += ch;
            else if (u % 3 == 0) mut += "ACGT"[rnd_below(4)];
            else if (u % 3 == 1) { mut += ch; mut += "ACGT"[rnd_below(4)]; }
        }
        const int at = rnd_below(n + (int)mut.size()) - (int)mut.size() + 1;     // may hang over either end
        for (int q = 0; q < (int)mut.size(); ++q) if (at + q >= 0 && at + q < n) r[at + q] = mut[q];
    }
    return r;
}

// exact copies of both adapters, apart, in random bases: at a floor of 100 % (F = match * m, no gap affordable) W_low is
// R - r0, and the copy's path needs every column of it -- the case that a window one block too short loses
std::string exact_copies(const std::string &a, const std::string &b)
{
    return random_bases(61) + a + random_bases(74) + b + random_bases(53);      // (one length for a pair of the same adapter twice)
}

long floor_of(const Scheme &s, int m, double threshold)
{
    const double t = (threshold - 1e-6) / 100.0;
    const int P = std::max(-s.mismatch, std::max(-s.open, -s.ext));
    const double per_base = t * s.match - P * (1.0 - t);
    return per_base <= 0 ? -1 : (long)(m * per_base);
}

}  // namespace

int main(int argc, char **argv)
{
    const int per_case = argc > 1 ? atoi(argv[1]) : 6;
    const Scheme schemes[3] = {{3, -6, -5, -2}, {3, -6, -2, -5}, {5, -4, -10, -1}};
    const char *y28 = "AATGTACTTCGTTCAGTTACGTATTGCT", *y22 = "GCAATACGTAACTGAACGAAGT", *a24 = "GGTTGTTTCTGTTGGTGCTGATAT",
               *a33 = "GCTTGGGTGTTTAACCGTTTTCGCATTTATCGT", *a30 = "CACAAAGACACCGACAACTTTCTTCAGCAC";
    const char *pairs[7][2] = {{y28, y22}, {a33, a30}, {y22, y22}, {a24, a24}, {y28, y28}, {a30, a30}, {a33, a33}};
    long bad = 0, pairs_n = 0, at_or_above = 0, below = 0, plans = 0, rule_r0s = 0, cols = 0, cols_on = 0;
    // refused schemes: a rewarded gap opening, a free gap extension, a free opening, linear gaps, match < mismatch
    const Scheme refused[5] = {{1, -100, 5, -1}, {3, -6, -5, 0}, {3, -6, 0, -2}, {3, -6, -5, -5}, {3, 4, -5, -2}};
    for (const Scheme &s : refused) {
        if (pcb::row_skip_plan(s.match, s.mismatch, s.open, s.ext, 28, 22, 28, 22, 46, 36).ok) { printf("BAD: scheme %d,%d,%d,%d accepted\n", s.match, s.mismatch, s.open, s.ext); ++bad; }
        if (pcb::row_skip_r0(s.match, s.mismatch, s.open, s.ext, 28, 28, 22) != 28) { printf("BAD: a row for a refused scheme\n"); ++bad; }
    }
    // refused rows and floors: odd, in the padding, the last row, a floor that leaves theta <= 0 (the column-0 condition)
    if (pcb::row_skip_plan(3, -6, -5, -2, 28, 21, 28, 22, 46, 36).ok || pcb::row_skip_plan(3, -6, -5, -2, 28, 6, 28, 22, 80, 60).ok ||
        pcb::row_skip_plan(3, -6, -5, -2, 28, 28, 28, 22, 46, 36).ok || pcb::row_skip_plan(3, -6, -5, -2, 28, 22, 28, 22, 46, 18).ok ||
        pcb::row_skip_plan(3, -6, -5, -2, 28, 22, 28, 22, 46, 17).ok || !pcb::row_skip_plan(3, -6, -5, -2, 28, 22, 28, 22, 46, 19).ok) {
        printf("BAD: row_skip_plan's refusals\n"); ++bad;
    }
    for (int si = 0; si < 3; ++si) {
        const Scheme &s = schemes[si];
        long s_above = 0, s_below = 0, s_plans = 0, s_rule = 0;
        for (const auto &pr : pairs) {
            const std::string ad[2] = {pr[0], pr[1]};
            const int m[2] = {(int)ad[0].size(), (int)ad[1].size()};
            const int R = std::max(m[0], m[1]);
            const int rule = pcb::row_skip_r0(s.match, s.mismatch, s.open, s.ext, R, m[0], m[1]);
            if (rule < R) { ++rule_r0s; ++s_rule; }
            for (double thr : {75.0, 85.0, 90.0, 100.0}) {
                const bool exact = thr == 100.0;
                const long F[2] = {exact ? (long)s.match * m[0] : floor_of(s, m[0], thr), exact ? (long)s.match * m[1] : floor_of(s, m[1], thr)};
                if (F[0] <= 0 || F[1] <= 0) continue;
                for (int w = 0; w < (exact ? 2 : per_case); ++w) {
                    // a dual tile reads one window with both adapters; two streams of one adapter read two windows
                    std::string rd[2];
                    rd[0] = exact ? exact_copies(ad[0], ad[1]) : make_read((w == 0) ? 0 : (w == 1) ? 1 + rnd_below(40) : rnd_below(601), ad[0], ad[1]);
                    rd[1] = (ad[0] != ad[1]) ? rd[0] : exact ? exact_copies(ad[1], ad[0]) : make_read((int)rd[0].size(), ad[0], ad[1]);
                    const int n = (int)rd[0].size();
                    const Matrix full[2] = {run(rd[0], ad[0], s, 1 << 20, nullptr, false), run(rd[1], ad[1], s, 1 << 20, nullptr, false)};
                    for (int r0 = 2; r0 < R; r0 += 2) {
                        const pcb::RowSkip p = pcb::row_skip_plan(s.match, s.mismatch, s.open, s.ext, R, r0, m[0], m[1], F[0], F[1]);
                        if (!p.ok) { if (r0 == rule && thr == 90.0) { printf("BAD: the rule's row refused at its own floor\n"); ++bad; } continue; }
                        ++plans; ++s_plans;
                        const int theta[2] = {p.theta_lo, p.theta_hi};
                        const int i0[2] = {r0 - (R - m[0]), r0 - (R - m[1])};       // row r0 in each adapter's own rows
                        // the window: columns j'' .. j'' + W_low behind a trigger in either stream
                        std::vector<char> on(n + 1, 0);
                        int until = -1;
                        for (int j = 0; j <= n; ++j) {
                            for (int h = 0; h < 2; ++h) if (j >= 1 && full[h].at(i0[h], j) >= theta[h]) until = j + p.w_low;
                            on[j] = j <= until;
                            ++cols; cols_on += on[j];
                        }
                        on[0] = 1;                                                // column 0 is the start state: M = 0 in every row
                        for (int h = 0; h < 2; ++h) {
                            const Matrix hat = run(rd[h], ad[h], s, i0[h], &on, false);
                            for (int j = 0; j <= n; ++j)
                                for (int i = 0; i <= m[h]; ++i) {
                                    const int a = hat.at(i, j), b = full[h].at(i, j);
                                    if (a > b) { if (bad < 20) printf("BAD claim 1: M^ %d > M %d at (%d,%d)\n", a, b, i, j); ++bad; }
                                    if (i <= i0[h] && a != b) { if (bad < 20) printf("BAD: an upper row differs at (%d,%d)\n", i, j); ++bad; }
                                    if ((j == n || i == m[h]) && j >= 1 && i >= 1 && b >= F[h] && a != b) {
                                        if (bad < 20) printf("BAD claim 2: M %d >= F %ld but M^ %d at (%d,%d) r0 %d\n", b, F[h], a, i, j, r0);
                                        ++bad;
                                    }
                                }
                            // claim 3: nothing at or above row r0, starts in column 0 only
                            const Matrix low = run(rd[h], ad[h], s, i0[h], nullptr, true);
                            for (int j = 0; j <= n; ++j)
                                for (int i = i0[h] + 1; i <= m[h]; ++i)
                                    if (low.at(i, j) > (long)s.match * (R - r0 - 1) || low.at(i, j) >= F[h]) {
                                        if (bad < 20) printf("BAD claim 3: %d at (%d,%d)\n", low.at(i, j), i, j);
                                        ++bad;
                                    }
                            int b0, I0, J0, b1, I1, J1;
                            scout(full[h], b0, I0, J0); scout(hat, b1, I1, J1);
                            if (b0 >= F[h]) { if (b1 != b0 || I1 != I0 || J1 != J0) { if (bad < 20) printf("BAD: end cell (%d,%d,%d) != (%d,%d,%d)\n", b1, I1, J1, b0, I0, J0); ++bad; } }
                            else if (b1 >= F[h]) { if (bad < 20) printf("BAD: a pair below F rose to %d\n", b1); ++bad; }
                            if (r0 == 2 * ((R - 4) / 2)) { ++pairs_n; if (b0 >= F[h]) { ++at_or_above; ++s_above; } else { ++below; ++s_below; } }
                        }
                    }
                }
            }
        }
        printf("scheme %d,%d,%d,%d plans=%ld at_or_above=%ld below=%ld rule_rows=%ld\n", s.match, s.mismatch, s.open, s.ext, s_plans, s_above, s_below, s_rule);
    }
    printf("pairs=%ld at_or_above=%ld below=%ld plans=%ld rule_rows=%ld columns=%ld columns_on=%ld bad=%ld \n", pairs_n, at_or_above, below, plans,
           rule_r0s, cols, cols_on, bad);
    return bad ? 1 : 0;
}
