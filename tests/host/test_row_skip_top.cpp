// test_row_skip_top.cpp -- the row-skip proposition of pc_bounds.h for the TOP-aligned layout (row_skip_plan_top) held,
// cell for cell, against the plain recurrence of pc_cell.h.  Host only.
//
// Two streams share a window of lower rows, as the two halves of a tile do.  Both adapters start in register row 1; the
// shorter one is followed by padding rows down to register row R, whose letter scores 0 against every base.  The skipping
// recurrence computes rows <= r0 in every column and rows > r0 only in the columns j'' .. j'' + W_low behind a column with
// M(r0, j'') >= theta in either stream; where the rows below are switched on their values of the column before are
// -infinity.  Each stream is run over all R register rows, padding included, as the kernel runs it.  Checked, for every
// even r0 row_skip_plan_top accepts, for floors of 75 / 85 / 90 % identity:
//   claim 0   the real rows of the padded matrix are those of the adapter alone: nothing reads a padding row
//   claim 1   M^ <= M in every cell (a cell that is not computed counts as -infinity), rows <= r0 are exact
//   claim 2   every candidate end cell (row m at any column, the last column at rows 1..m) with M >= F has M^ = M
//   (and once per pair at the floor of 100 %, F = match * m, on exact copies: there the window is m - r0 and the copy's path
//   needs every column of it, and M(r0, j'') is theta exactly)
//   claim 3   a path that starts in column 0 below row r0 scores at most match * (m - r0 - 1) < F
//   and the consequences: the scout over rows 1..m picks the same end cell whenever the true best is >= F; a pair below F
//   stays below.  Over a whole window a padding row's last-column cell never beats the real candidates (it carries a
//   last-row value of an earlier column on, and that one is a candidate itself); behind a chunk's untracked lead-in it
//   does: the third window of every case of unequal lengths ends k <= R - m columns behind an exact copy of the shorter
//   adapter and tracks only those k columns.  A scout that also took the padding rows would answer with the copy's
//   score there: counted (pad_would_win) and required to have happened, so that the exclusion is tested and not assumed.
// Also: the refusals, the equality of both plans for equal lengths, the rule's rows for the two headline pairs.
//   usage: test_row_skip_top [windows per case]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pc_bounds.h"
#include "pc_cell.h"
#include "pc_letters.h"

namespace {

uint64_t g_state = 0x2545F4914F6CDD1Dull;
uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
int rnd_below(int n) { return n > 0 ? (int)(rnd() % (uint32_t)n) : 0; }

struct Scheme { int match, mismatch, open, ext; };
constexpr char kPad = '#';                                           // the padding row's letter: scores 0 against everything

// M of every cell, rows 0..m (m = the rows given, padding included), columns 0..n; on[j] says whether rows > i0 are computed
// in column j.  A cell that is not computed holds -infinity in all three states.
struct Matrix { int n, m; std::vector<int> M; int at(int i, int j) const { return M[(size_t)j * (m + 1) + i]; } };

Matrix run(const std::string &read, const std::string &rows, const Scheme &s, int i0, const std::vector<char> *on, bool only_below)
{
    const int n = (int)read.size(), m = (int)rows.size();
    Matrix x{n, m, std::vector<int>((size_t)(n + 1) * (m + 1), pcc::NEG_INF)};
    std::vector<int> Mc(m + 1, 0), Hc(m + 1, pcc::NEG_INF);          // the column state: M = 0 in column 0, H = -inf
    auto off = [&](int i, int j) { return (on && i > i0 && !(*on)[j]) || (only_below && i <= i0); };
    for (int i = 0; i <= m; ++i) {
        if (only_below && i <= i0) Mc[i] = pcc::NEG_INF;             // claim 3's matrix: no start at or above row i0
        x.M[i] = Mc[i];
    }
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
            const int sub = rows[i - 1] == kPad ? 0 : (h == pcc::dna5_code((uint8_t)rows[i - 1])) ? s.match : s.mismatch;
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

// the scout over the candidate cells of rows 1..m_real, in visiting order (last row = m_real; the last column's rows down to
// `through`: m_real as the kernel has it, the register rows' R for the scout that wrongly takes padding rows); tf: the columns
// <= tf are a chunk's lead-in and are not tracked (pc_jit_source.h: tf_lo / tf_hi; 0 for a whole window)
void scout(const Matrix &x, int m_real, int through, int tf, int &best, int &I, int &J)
{
    best = tf > 0 ? pcc::NEG_INF : 0; I = m_real; J = tf > 0 ? -1 : 0;     // (m, 0) belongs to the chunk that starts at column 0
    for (int j = tf + 1; j <= x.n; ++j)
        for (int i = 1; i <= through; ++i)
            if ((j == x.n || i == m_real) && x.at(i, j) > best) { best = x.at(i, j); I = i; J = j; }
}

std::string random_bases(int n) { std::string r(n, 'A'); for (char &c : r) c = "ACGT"[rnd_below(4)]; return r; }

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

std::string exact_copies(const std::string &a, const std::string &b)
{
    return random_bases(61) + a + random_bases(74) + b + random_bases(53);
}

long floor_of(const Scheme &s, int m, double threshold)
{
    const double t = (threshold - 1e-6) / 100.0;
    const int P = std::max(-s.mismatch, std::max(-s.open, -s.ext));
    const double per_base = t * s.match - P * (1.0 - t);
    return per_base <= 0 ? -1 : (long)(m * per_base);
}

bool same_plan(const pcb::RowSkip &a, const pcb::RowSkip &b)
{
    return a.ok == b.ok && a.theta_lo == b.theta_lo && a.theta_hi == b.theta_hi && a.w_low == b.w_low;
}

int rule_row(const Scheme &s, const std::string &a, const std::string &b)
{
    unsigned char sa[pcb::MAX_ADAPTER], sb[pcb::MAX_ADAPTER];
    for (size_t i = 0; i < a.size(); ++i) sa[i] = (unsigned char)pcl::letter_set((uint8_t)a[i], false);
    for (size_t i = 0; i < b.size(); ++i) sb[i] = (unsigned char)pcl::letter_set((uint8_t)b[i], false);
    const int R = (int)std::max(a.size(), b.size());
    return pcb::row_skip_r0_top(s.match, s.mismatch, s.open, s.ext, R, (int)a.size(), (int)b.size(), sa, sb);
}

}  // namespace

int main(int argc, char **argv)
{
    const int per_case = argc > 1 ? atoi(argv[1]) : 6;
    const Scheme schemes[3] = {{3, -6, -5, -2}, {3, -6, -2, -5}, {5, -4, -10, -1}};
    const std::string y28 = "AATGTACTTCGTTCAGTTACGTATTGCT", y22 = "GCAATACGTAACTGAACGAAGT", a24 = "GGTTGTTTCTGTTGGTGCTGATAT",
                      a33 = "GCTTGGGTGTTTAACCGTTTTCGCATTTATCGT", a30 = "CACAAAGACACCGACAACTTTCTTCAGCAC", a14 = a24.substr(0, 14);
    // the two headline pairs (either order of the halves), a pair with a large length gap (28 | 14: K_up = 12, three waves), an
    // equal-length pair
    const std::string pairs[6][2] = {{y28, y22}, {a33, a30}, {y22, y28}, {y28, a14}, {a14, y28}, {a24, a24}};
    long bad = 0, pairs_n = 0, at_or_above = 0, below = 0, plans = 0, cols = 0, cols_on = 0, pad_would_win = 0;
    // refused schemes: a rewarded gap opening, a free gap extension, a free opening, linear gaps, match < mismatch
    const Scheme refused[5] = {{1, -100, 5, -1}, {3, -6, -5, 0}, {3, -6, 0, -2}, {3, -6, -5, -5}, {3, 4, -5, -2}};
    for (const Scheme &s : refused) {
        if (pcb::row_skip_plan_top(s.match, s.mismatch, s.open, s.ext, 28, 18, 28, 22, 58, 46).ok) { printf("BAD: scheme %d,%d,%d,%d accepted\n", s.match, s.mismatch, s.open, s.ext); ++bad; }
        if (rule_row(s, y28, y22) != 28) { printf("BAD: a row for a refused scheme\n"); ++bad; }
    }
    // refused rows and floors: odd; r0 >= min(m) (22, 24: at or below the short half's last row); r0 = 0; a floor that leaves
    // theta <= 0 in the short half (46 - 3 * 4 > 0, but 12 - 12 = 0 and 11 - 12 < 0) or in the long half (30 - 30 = 0); a floor
    // above match * m.  And the row just inside every limit is accepted.
    auto top = [](int r0, long Flo, long Fhi) { return pcb::row_skip_plan_top(3, -6, -5, -2, 28, r0, 28, 22, Flo, Fhi).ok; };
    if (top(19, 58, 46) || top(22, 58, 46) || top(24, 58, 46) || top(0, 58, 46) || top(18, 58, 12) || top(18, 58, 11) || top(18, 30, 46) ||
        top(18, 85, 46) || top(18, 58, 67) || !top(20, 58, 46) || !top(18, 58, 13) || !top(18, 31, 46) || !top(18, 84, 66) || !top(2, 84, 66)) {
        printf("BAD: row_skip_plan_top's refusals\n"); ++bad;
    }
    // (the halves in the other order: the same plan with the thresholds swapped)
    {
        const pcb::RowSkip p = pcb::row_skip_plan_top(3, -6, -5, -2, 28, 18, 28, 22, 58, 46), q = pcb::row_skip_plan_top(3, -6, -5, -2, 28, 18, 22, 28, 46, 58);
        // theta = 58 - 30 | 46 - 12; W_low = max(10 + 26 / 2, 4 + 20 / 2)
        if (!p.ok || p.theta_lo != 28 || p.theta_hi != 34 || p.w_low != 23 || !q.ok || q.theta_lo != 34 || q.theta_hi != 28 || q.w_low != 23) { printf("BAD: the plan of 28 | 22 at row 18\n"); ++bad; }
    }
    // equal lengths: both layouts are one, the plans agree in every field -- every row, floors all over the range
    for (const Scheme &s : schemes)
        for (int m : {22, 24, 33})
            for (int r0 = 0; r0 <= m + 1; ++r0)
                for (long F = -3; F <= (long)s.match * m + 3; F += 1 + (F & 3))
                    for (long dF : {0L, 5L}) {
                        if (!same_plan(pcb::row_skip_plan_top(s.match, s.mismatch, s.open, s.ext, m, r0, m, m, F, F - dF),
                                       pcb::row_skip_plan(s.match, s.mismatch, s.open, s.ext, m, r0, m, m, F, F - dF))) {
                            if (bad < 20) printf("BAD: the plans of an equal-length pair differ (m %d r0 %d F %ld)\n", m, r0, F);
                            ++bad;
                        }
                    }
    // the rule's rows for the two headline pairs at the default scores: what the shipped kernels are compiled with
    printf("rule 28|22=%d 33|30=%d\n", rule_row(schemes[0], y28, y22), rule_row(schemes[0], a33, a30));
    for (int si = 0; si < 3; ++si) {
        const Scheme &s = schemes[si];
        long s_above = 0, s_below = 0, s_plans = 0;
        for (const auto &pr : pairs) {
            const std::string ad[2] = {pr[0], pr[1]};
            const int m[2] = {(int)ad[0].size(), (int)ad[1].size()};
            const int R = std::max(m[0], m[1]);
            const std::string rows[2] = {ad[0] + std::string(R - m[0], kPad), ad[1] + std::string(R - m[1], kPad)};
            for (double thr : {75.0, 85.0, 90.0, 100.0}) {
                const bool exact = thr == 100.0;
                const long F[2] = {exact ? (long)s.match * m[0] : floor_of(s, m[0], thr), exact ? (long)s.match * m[1] : floor_of(s, m[1], thr)};
                if (F[0] <= 0 || F[1] <= 0) continue;
                for (int w = 0; w < (exact ? 2 : per_case); ++w) {
                    std::string rd[2];
                    rd[0] = exact ? exact_copies(ad[0], ad[1]) : make_read((w == 0) ? 0 : (w == 1) ? 1 + rnd_below(40) : rnd_below(601), ad[0], ad[1]);
                    rd[1] = (ad[0] != ad[1]) ? rd[0] : exact ? exact_copies(ad[1], ad[0]) : make_read((int)rd[0].size(), ad[0], ad[1]);
                    int tf = 0;
                    if (!exact && w == 2 && m[0] != m[1]) {                       // the padding rows' case (see the head of the file)
                        const int k = 1 + rnd_below(R - std::min(m[0], m[1]));
                        rd[0] = rd[1] = random_bases(30 + rnd_below(60)) + (m[0] < m[1] ? ad[0] : ad[1]) + random_bases(k);
                        tf = (int)rd[0].size() - k;
                    }
                    const int n = (int)rd[0].size();
                    const Matrix full[2] = {run(rd[0], rows[0], s, 1 << 20, nullptr, false), run(rd[1], rows[1], s, 1 << 20, nullptr, false)};
                    for (int h = 0; h < 2; ++h) {                                 // claim 0
                        const Matrix alone = run(rd[h], ad[h], s, 1 << 20, nullptr, false);
                        for (int j = 0; j <= n; ++j)
                            for (int i = 0; i <= m[h]; ++i)
                                if (alone.at(i, j) != full[h].at(i, j)) { if (bad < 20) printf("BAD claim 0: a real row reads the padding at (%d,%d)\n", i, j); ++bad; }
                        int b0, I0, J0, b2, I2, J2;
                        scout(full[h], m[h], m[h], tf, b0, I0, J0); scout(full[h], m[h], R, tf, b2, I2, J2);
                        if (I2 > m[h]) ++pad_would_win;
                    }
                    for (int r0 = 2; r0 < R; r0 += 2) {
                        const pcb::RowSkip p = pcb::row_skip_plan_top(s.match, s.mismatch, s.open, s.ext, R, r0, m[0], m[1], F[0], F[1]);
                        if (!p.ok) continue;
                        if (r0 >= std::min(m[0], m[1])) { printf("BAD: row %d accepted at or below a last row\n", r0); ++bad; continue; }
                        ++plans; ++s_plans;
                        const int theta[2] = {p.theta_lo, p.theta_hi};
                        std::vector<char> on(n + 1, 0);
                        int until = -1;
                        for (int j = 0; j <= n; ++j) {
                            for (int h = 0; h < 2; ++h) if (j >= 1 && full[h].at(r0, j) >= theta[h]) until = j + p.w_low;
                            on[j] = j <= until;
                            ++cols; cols_on += on[j];
                        }
                        on[0] = 1;                                                // column 0 is the start state: M = 0 in every row
                        for (int h = 0; h < 2; ++h) {
                            const Matrix hat = run(rd[h], rows[h], s, r0, &on, false);
                            for (int j = 0; j <= n; ++j)
                                for (int i = 0; i <= m[h]; ++i) {
                                    const int a = hat.at(i, j), b = full[h].at(i, j);
                                    if (a > b) { if (bad < 20) printf("BAD claim 1: M^ %d > M %d at (%d,%d)\n", a, b, i, j); ++bad; }
                                    if (i <= r0 && a != b) { if (bad < 20) printf("BAD: an upper row differs at (%d,%d)\n", i, j); ++bad; }
                                    if ((j == n || i == m[h]) && j >= 1 && i >= 1 && b >= F[h] && a != b) {
                                        if (bad < 20) printf("BAD claim 2: M %d >= F %ld but M^ %d at (%d,%d) r0 %d half %d\n", b, F[h], a, i, j, r0, h);
                                        ++bad;
                                    }
                                }
                            const Matrix low = run(rd[h], ad[h], s, r0, nullptr, true);   // claim 3
                            for (int j = 0; j <= n; ++j)
                                for (int i = r0 + 1; i <= m[h]; ++i)
                                    if (low.at(i, j) > (long)s.match * (m[h] - r0 - 1) || low.at(i, j) >= F[h]) {
                                        if (bad < 20) printf("BAD claim 3: %d at (%d,%d)\n", low.at(i, j), i, j);
                                        ++bad;
                                    }
                            int b0, I0, J0, b1, I1, J1;
                            scout(full[h], m[h], m[h], tf, b0, I0, J0); scout(hat, m[h], m[h], tf, b1, I1, J1);
                            if (b0 >= F[h]) { if (b1 != b0 || I1 != I0 || J1 != J0) { if (bad < 20) printf("BAD: end cell (%d,%d,%d) != (%d,%d,%d)\n", b1, I1, J1, b0, I0, J0); ++bad; } }
                            else if (b1 >= F[h]) { if (bad < 20) printf("BAD: a pair below F rose to %d\n", b1); ++bad; }
                            if (r0 == 2 * ((std::min(m[0], m[1]) - 1) / 2)) { ++pairs_n; if (b0 >= F[h]) { ++at_or_above; ++s_above; } else { ++below; ++s_below; } }
                        }
                    }
                }
            }
        }
        printf("scheme %d,%d,%d,%d plans=%ld at_or_above=%ld below=%ld\n", s.match, s.mismatch, s.open, s.ext, s_plans, s_above, s_below);
    }
    printf("pairs=%ld at_or_above=%ld below=%ld plans=%ld columns=%ld columns_on=%ld pad_would_win=%ld bad=%ld \n", pairs_n, at_or_above, below, plans,
           cols, cols_on, pad_would_win, bad);
    return bad ? 1 : 0;
}
