// Host check of porechop_amd/csrc/pc_end_rule.h against the oracle: a pair the rule rejects from its score record
// (score, end cell) and window length must not trim its read by the reference's condition (nanopore_read.py:166-208, as
// tests/ref_pipeline.py states it), and the rule's bound must hold for the pairs it keeps.  Seeded random windows of 0 to 150
// bases against adapters of 22, 24, 28, 30 and 33 bases: the adapter planted at the window's start, at its end, in the middle,
// cut by either edge, mutated to 60-100 % identity, and absent; three scoring schemes; start and end windows.
// usage: test_end_rule [repetitions per (scheme, adapter, side, case)]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

#include "pc_end_rule.h"
#include "pc_oracle.h"

namespace {

const int kSchemes[3][4] = {{3, -6, -5, -2}, {3, -6, -2, -5}, {4, -7, -10, -140}};
const int kAdapterLens[5] = {22, 24, 28, 30, 33};
const double kThresholds[2] = {75.0, 90.0};
enum Case { AT_START, AT_END, MIDDLE, CUT_LEFT, CUT_RIGHT, MUTATED, ABSENT, NCASES };
const char *const kCaseNames[NCASES] = {"at_start", "at_end", "middle", "cut_left", "cut_right", "mutated", "absent"};

std::mt19937 rng(20261019u);
int randint(int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); }
char base() { return "ACGT"[rng() & 3]; }
std::string bases(int n) { std::string s; for (int i = 0; i < n; ++i) s.push_back(base()); return s; }

// a copy of `ad` at about `identity` (0.6 .. 1.0): substitutions, deletions and insertions
std::string mutate(const std::string &ad, double identity)
{
    std::string s;
    for (char ch : ad) {
        if ((rng() % 10000) / 10000.0 < identity) { s.push_back(ch); continue; }
        switch (rng() % 3) {
            case 0: { char c; do c = base(); while (c == ch); s.push_back(c); break; }
            case 1: break;
            default: s.push_back(ch); s.push_back(base());
        }
    }
    return s;
}

std::string make_window(Case c, const std::string &ad, int n)
{
    const int m = (int)ad.size();
    std::string w = bases(n);
    auto put = [&](int at, const std::string &copy) {          // copy[k] -> w[at + k] where that lies inside the window
        for (int k = 0; k < (int)copy.size(); ++k) if (at + k >= 0 && at + k < n) w[at + k] = copy[k];
    };
    switch (c) {
        case AT_START: put(0, ad); break;
        case AT_END: put(n - m, ad); break;
        case MIDDLE: put(n > m ? randint(1, n - m) : 0, ad); break;
        case CUT_LEFT: put(-randint(1, m - 1), ad); break;
        case CUT_RIGHT: put(n - randint(1, m - 1), ad); break;
        case MUTATED: {
            const std::string copy = mutate(ad, 0.6 + 0.4 * ((rng() % 1001) / 1000.0));
            put(randint(-4, n > (int)copy.size() ? n - (int)copy.size() + 4 : 4), copy);
            break;
        }
        default: break;
    }
    return w;
}

}  // namespace

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? atoi(argv[1]) : 40;
    const int end_size = 150, min_trim_size = 4, extra_end_trim = 2;
    long bad = 0, pairs = 0;
    for (int si = 0; si < 3; ++si) {
        const int *sc = kSchemes[si];
        long rejected = 0, accepted = 0, trimming = 0, rejected_by_case[NCASES] = {0};
        for (double threshold : kThresholds) {
            const pcr::EndRule rule = pcr::make_end_rule(sc[0], sc[1], sc[2], sc[3], end_size, min_trim_size, extra_end_trim, threshold);
            for (int m : kAdapterLens) {
                const std::string ad = bases(m);
                for (int side = 0; side < 2; ++side) for (int c = 0; c < NCASES; ++c) for (int rep = 0; rep < reps; ++rep) {
                    // windows of every length from 0 to 150, the full window -- what most reads give -- every third time
                    const int n = rep % 3 == 0 ? end_size : randint(0, end_size);
                    const std::string w = make_window((Case)c, ad, n);
                    pc_oracle_result r;
                    if (pc_oracle_align_raw(w.data(), n, ad.data(), m, sc[0], sc[1], sc[2], sc[3], &r) != 0) { printf("oracle failed\n"); return 2; }
                    ++pairs;
                    // the reference's trim of this pair (tests/ref_pipeline.py phase_b): from the 7-field string, as the caller reads it
                    long trim = 0;
                    if (!r.failed) {
                        char buf[256];
                        pc_oracle_format(&r, buf, sizeof buf);
                        int rs = 0, re_incl = 0, as = 0, ae = 0, len = 0;
                        double partial = 0.0, full = 0.0;
                        if (sscanf(buf, "%d,%d,%d,%d,%d,%lf,%lf", &rs, &re_incl, &as, &ae, &len, &partial, &full) != 7) { printf("unreadable record %s\n", buf); return 2; }
                        const int re = re_incl + 1;
                        if (side == 0) {
                            if (partial > threshold && re != end_size && re - rs >= min_trim_size) trim = re + extra_end_trim;
                        } else {
                            if (partial > threshold && rs != 0 && re - rs >= min_trim_size) trim = (end_size - rs) + extra_end_trim;
                        }
                        if (trim < 0) trim = 0;                      // (a trim is a maximum that starts at 0)
                    }
                    // the score record the first pass writes for the pair: (-2, Jc, I, 0, S, ...) with the scout's end cell
                    const int flag = -2, S = r.failed ? 0 : r.score, I = r.failed ? 0 : r.end_i, Jc = r.failed ? 0 : r.end_j;
                    const long ub = (long)pcr::trim_bound(rule, side, flag, S, I, Jc, n, m);
                    const bool keep = pcr::can_trim(rule, side, flag, S, I, Jc, n, m);
                    if (keep != (ub > 0)) { ++bad; printf("BAD can_trim and trim_bound disagree\n"); }
                    if (trim > 0) ++trimming;
                    if (!keep) {
                        ++rejected; ++rejected_by_case[c];
                        if (trim != 0) {
                            ++bad;
                            printf("BAD rejected pair trims: scheme %d threshold %.0f m %d side %d case %s n %d S %d I %d Jc %d trim %ld\n  %s\n  %s\n",
                                   si, threshold, m, side, kCaseNames[c], n, S, I, Jc, trim, w.c_str(), ad.c_str());
                        }
                    } else {
                        ++accepted;
                        if (trim > ub) {
                            ++bad;
                            printf("BAD bound below the trim: scheme %d threshold %.0f m %d side %d case %s n %d S %d I %d Jc %d trim %ld ub %ld\n",
                                   si, threshold, m, side, kCaseNames[c], n, S, I, Jc, trim, ub);
                        }
                    }
                }
            }
        }
        // anything that is not a plain score record is traced
        const pcr::EndRule rule = pcr::make_end_rule(sc[0], sc[1], sc[2], sc[3], end_size, min_trim_size, extra_end_trim, 75.0);
        if (!pcr::can_trim(rule, 0, -1, 0, 0, 0, 150, 28) || !pcr::can_trim(rule, 1, 17, 5, 3, 2, 150, 28) || !pcr::can_trim(rule, 1, -2, 5, 40, 2, 150, 28) ||
            !pcr::can_trim(rule, 0, -2, 5, 3, 151, 150, 28)) { ++bad; printf("BAD an odd record was not kept for the traced pass\n"); }
        printf("scheme %d,%d,%d,%d: rejected=%ld accepted=%ld trimming=%ld  rejected by case:", sc[0], sc[1], sc[2], sc[3], rejected, accepted, trimming);
        for (int c = 0; c < NCASES; ++c) printf(" %s=%ld", kCaseNames[c], rejected_by_case[c]);
        printf("\n");
        // the rule neither traces everything nor nothing, and the cases do hold pairs that trim
        if (rejected == 0 || accepted == 0 || trimming == 0 || trimming >= accepted + rejected) { ++bad; printf("BAD scheme %d: a one-sided test\n", si); }
    }
    printf("pairs=%ld bad=%ld \n", pairs, bad);
    return bad ? 1 : 0;
}
