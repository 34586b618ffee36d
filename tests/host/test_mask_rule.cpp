// Host check of porechop_amd/csrc/pc_mask_rule.h against the oracle: after a stretch [rs, re) of a read is masked with '-',
// no pair's score rises, every record the rule keeps is the oracle's record of the masked read field for field and as the
// formatted string, and a pair below a score floor stays below it.  Seeded reads of 40 to 400 bases with 0 to 3 planted
// copies (0 / 5 / 15 / 30 % mutated) of the four headline adapters -- the 28- and 22-mer of SQK-NSK007, the 33- and 30-mer
// that share 22 bases with them -- and two 24-mer barcodes; three scoring schemes.  Masks: a record's own interval (what phase
// C masks), a random interval, two masks one after the other (the second on a read that already holds '-'), and intervals
// that meet a record's interval by exactly 0 and 1 columns on either side.  The gate: an adapter with N, wildcards on and
// mismatch > match are refused, and the case that shows why is here (47 -> 81).
// usage: test_mask_rule [reads per scheme]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "pc_mask_rule.h"
#include "pc_oracle.h"

namespace {

const int kSchemes[3][4] = {{3, -6, -5, -2}, {3, -6, -2, -5}, {4, -7, -10, -140}};
const char *const kAdapters[6] = {"AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT", "CTTCGTTCAGTTACGTATTGCTGGCGTCTGCTT",
                                  "CACCCAAGCAGACGCCAGCAATACGTAACT", "AAGAAAGTTGTCGGTGTCTTTGTG", "TCGATTCCGTTTGTAGTCGTCTGT"};
const int kNumAdapters = 6;
const double kMutation[4] = {0.0, 0.05, 0.15, 0.30};
const double kThresholds[3] = {75.0, 85.0, 90.0};

std::mt19937 rng(20261020u);
int randint(int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); }
char base() { return "ACGT"[rng() & 3]; }
std::string bases(int n) { std::string s; for (int i = 0; i < n; ++i) s.push_back(base()); return s; }

std::string mutate(const std::string &ad, double rate)
{
    std::string s;
    for (char ch : ad) {
        if ((rng() % 10000) / 10000.0 >= rate) { s.push_back(ch); continue; }
        switch (rng() % 3) {
            case 0: { char c; do c = base(); while (c == ch); s.push_back(c); break; }
            case 1: break;
            default: s.push_back(ch); s.push_back(base());
        }
    }
    return s;
}

std::string make_read()
{
    const int n = randint(40, 400);
    std::string r = bases(n);
    const int copies = randint(0, 3);
    for (int c = 0; c < copies; ++c) {
        const std::string copy = mutate(kAdapters[randint(0, kNumAdapters - 1)], kMutation[randint(0, 3)]);
        const int at = randint(-6, n - (int)copy.size() + 6);           // (now and then cut by an end of the read)
        for (int k = 0; k < (int)copy.size(); ++k) if (at + k >= 0 && at + k < n) r[at + k] = copy[k];
    }
    return r;
}

pc_oracle_result align(const std::string &read, const char *ad, const int *sc)
{
    pc_oracle_result r;
    if (pc_oracle_align_raw(read.data(), (int)read.size(), ad, (int)strlen(ad), sc[0], sc[1], sc[2], sc[3], &r) != 0) { printf("oracle failed\n"); exit(2); }
    return r;
}

std::string masked(const std::string &read, int rs, int re)
{
    std::string m = read;
    for (int j = rs < 0 ? 0 : rs; j < re && j < (int)m.size(); ++j) m[j] = '-';
    return m;
}

// Pipeline.identity_score_bound: the smallest score of an alignment of an m-base adapter whose identity reaches the threshold; 0: none
int score_floor(int m, double threshold, const int *sc)
{
    const double t = (threshold - 1e-6) / 100.0;
    int P = -sc[1];
    if (-sc[2] > P) P = -sc[2];
    if (-sc[3] > P) P = -sc[3];
    const double per_base = t * sc[0] - P * (1.0 - t);
    if (per_base <= 0) return 0;
    return (int)(m * per_base);
}

bool same_record(const pc_oracle_result &a, const pc_oracle_result &b)
{
    if (a.failed != b.failed) return false;
    if (a.failed) return true;
    char sa[256], sb[256];
    pc_oracle_format(&a, sa, sizeof sa);
    pc_oracle_format(&b, sb, sizeof sb);
    return a.read_start == b.read_start && a.read_end == b.read_end && a.adapter_start == b.adapter_start && a.adapter_end == b.adapter_end &&
           a.score == b.score && a.aligned_matches == b.aligned_matches && a.aligned_len == b.aligned_len && a.full_matches == b.full_matches &&
           a.full_len == b.full_len && a.path_len == b.path_len && a.end_i == b.end_i && a.end_j == b.end_j && strcmp(sa, sb) == 0;
}

struct Tally { long cases = 0, kept = 0, realigned = 0, below_floor = 0, bad = 0; };

// One mask [rs, re) over `read`: every adapter before and after.
void check_mask(const std::string &read, int rs, int re, const int *sc, Tally &t, const char *what)
{
    const std::string after_read = masked(read, rs, re);
    for (int a = 0; a < kNumAdapters; ++a) {
        const pc_oracle_result before = align(read, kAdapters[a], sc), after = align(after_read, kAdapters[a], sc);
        ++t.cases;
        if (before.failed || after.failed) {
            if (before.failed != after.failed) { ++t.bad; printf("BAD %s: a failed record on one side only\n", what); }
            continue;
        }
        if (after.score > before.score) {
            ++t.bad;
            printf("BAD %s: the score rose %d -> %d (adapter %d, mask %d-%d)\n  %s\n", what, before.score, after.score, a, rs, re, read.c_str());
        }
        // the rule, asked as the rounds ask it: an adapter above the one that hit, unfloored
        const bool realign = pcm::must_realign(1, 0, before.read_start, before.read_end, rs, re, false);
        if (realign) {
            ++t.realigned;
        } else {
            ++t.kept;
            if (!same_record(before, after)) {
                char sa[256], sb[256];
                pc_oracle_format(&before, sa, sizeof sa);
                pc_oracle_format(&after, sb, sizeof sb);
                ++t.bad;
                printf("BAD %s: a kept record changed (adapter %d, mask %d-%d)\n  %s\n  %s\n  %s\n", what, a, rs, re, sa, sb, read.c_str());
            }
        }
        // floors at the bounds of 75 / 85 / 90 %: below stays below, and the floored rule keeps the "no alignment" record
        for (double thr : kThresholds) {
            const int F = score_floor((int)strlen(kAdapters[a]), thr, sc);
            if (F <= 0 || before.score >= F) continue;
            ++t.below_floor;
            if (after.score >= F) { ++t.bad; printf("BAD %s: a pair below its floor %d reached it: %d -> %d\n", what, F, before.score, after.score); }
            if (pcm::must_realign(1, 0, -1, 0, rs, re, true)) { ++t.bad; printf("BAD the floored rule realigns a 'no alignment' record\n"); }
        }
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const int reads = argc > 1 ? atoi(argv[1]) : 150;
    long bad = 0, cases = 0;

    // ---- the rule's fixed answers
    if (pcm::must_realign(2, 3, 10, 20, 0, 100, false)) { ++bad; printf("BAD an adapter below the cursor is realigned\n"); }
    if (!pcm::must_realign(3, 3, 500, 520, 0, 100, true)) { ++bad; printf("BAD the hit adapter is not realigned\n"); }
    if (!pcm::must_realign(4, 3, -1, 0, 0, 100, false)) { ++bad; printf("BAD an unfloored 'no alignment' record is kept\n"); }
    if (pcm::must_realign(4, 3, -1, 0, 0, 100, true)) { ++bad; printf("BAD a floored 'no alignment' record is realigned\n"); }
    if (pcm::must_realign(4, 3, 10, 20, 15, 15, false)) { ++bad; printf("BAD an empty mask realigns\n"); }
    if (!pcm::must_realign(4, 3, 20, 10, 0, 100, false)) { ++bad; printf("BAD an odd record is kept\n"); }
    // touching by 0 and 1 columns, either side: record [10, 20], masks [rs, re)
    if (pcm::must_realign(4, 3, 10, 20, 5, 10, false) || !pcm::must_realign(4, 3, 10, 20, 5, 11, false) ||
        pcm::must_realign(4, 3, 10, 20, 21, 30, false) || !pcm::must_realign(4, 3, 10, 20, 20, 30, false)) { ++bad; printf("BAD the overlap test is off by a column\n"); }

    // ---- the gate, and why it is needed
    {
        const int lens6[6] = {28, 22, 33, 30, 24, 24};
        if (!pcm::gate(kAdapters, lens6, 6, 3, -6, -5, -2, false)) { ++bad; printf("BAD the gate refuses the plain adapters\n"); }
        if (pcm::gate(kAdapters, lens6, 6, 3, -6, -5, -2, true)) { ++bad; printf("BAD the gate accepts wildcards\n"); }
        if (pcm::gate(kAdapters, lens6, 6, 3, 4, -5, -2, false)) { ++bad; printf("BAD the gate accepts mismatch > match\n"); }
        if (!pcm::gate(kAdapters, lens6, 6, 3, 3, -5, -2, false)) { ++bad; printf("BAD the gate refuses mismatch == match\n"); }
        const char *const lower[1] = {"aatgtacuUCGT"};
        const int len_lower[1] = {12};
        if (!pcm::gate(lower, len_lower, 1, 3, -6, -5, -2, false)) { ++bad; printf("BAD the gate refuses lower case and U\n"); }
        const char *const with_n[2] = {kAdapters[0], "AATGTACTNNNNCAGTTACGTATTGCT"};
        const int len_n[2] = {28, 27};
        if (pcm::gate(with_n, len_n, 2, 3, -6, -5, -2, false)) { ++bad; printf("BAD the gate accepts an adapter with N\n"); }
        for (const char *odd : {"ACGT-ACGT", "ACGTRACGT", "ACG ACGT"}) {
            const char *const one[1] = {odd};
            const int len1[1] = {(int)strlen(odd)};
            if (pcm::gate(one, len1, 1, 3, -6, -5, -2, false)) { ++bad; printf("BAD the gate accepts %s\n", odd); }
        }
        // N equals N and '-' codes as N: the read holds the adapter's concrete copy, the mask covers the four bases under its N's
        const std::string read = std::string("GATTACAGATTACAGATTAC") + "AATGTACTTCGTCAGTTACGTATTGCT" + "CATTAGACATTAGACATTAG";
        const pc_oracle_result b = align(read, with_n[1], kSchemes[0]), a = align(masked(read, 28, 32), with_n[1], kSchemes[0]);
        printf("the N adapter: %d -> %d\n", b.score, a.score);
        if (b.score != 47 || a.score != 81) { ++bad; printf("BAD the case that shows why the gate is needed reads %d -> %d, not 47 -> 81\n", b.score, a.score); }
    }

    // ---- the claim against the oracle
    for (int si = 0; si < 3; ++si) {
        const int *sc = kSchemes[si];
        Tally t;
        for (int rep = 0; rep < reads; ++rep) {
            const std::string read = make_read();
            const int n = (int)read.size();
            std::vector<pc_oracle_result> rec;
            for (int a = 0; a < kNumAdapters; ++a) rec.push_back(align(read, kAdapters[a], sc));
            // (a) a record's own interval
            const pc_oracle_result &own = rec[randint(0, kNumAdapters - 1)];
            if (!own.failed) check_mask(read, own.read_start, own.read_end + 1, sc, t, "own interval");
            // (b) a random interval
            { const int rs = randint(0, n - 1); check_mask(read, rs, randint(rs, n < rs + 60 ? n : rs + 60), sc, t, "random interval"); }
            // (c) two masks one after the other: the second runs on a read that already holds '-'
            {
                const pc_oracle_result &first = rec[randint(0, kNumAdapters - 1)];
                const std::string once = first.failed ? masked(read, 0, n / 4) : masked(read, first.read_start, first.read_end + 1);
                const pc_oracle_result second = align(once, kAdapters[randint(0, kNumAdapters - 1)], sc);
                if (!second.failed) check_mask(once, second.read_start, second.read_end + 1, sc, t, "second mask");
                const int rs = randint(0, n - 1);
                check_mask(once, rs, randint(rs, n < rs + 60 ? n : rs + 60), sc, t, "second mask, random");
            }
            // (d) masks that meet a record's interval by exactly 0 and 1 columns, on either side
            {
                const pc_oracle_result &tr = rec[rep % kNumAdapters];
                if (!tr.failed) {
                    const int s = tr.read_start, e = tr.read_end;                 // inclusive
                    const int w = randint(1, 30);
                    if (s > 0) check_mask(read, s - w < 0 ? 0 : s - w, s, sc, t, "left, 0 columns");
                    check_mask(read, s - w < 0 ? 0 : s - w, s + 1, sc, t, "left, 1 column");
                    if (e + 1 < n) check_mask(read, e + 1, e + 1 + w > n ? n : e + 1 + w, sc, t, "right, 0 columns");
                    check_mask(read, e, e + 1 + w > n ? n : e + 1 + w, sc, t, "right, 1 column");
                }
            }
        }
        const long judged = t.kept + t.realigned;
        int floors = 0;                                   // (adapter, threshold) pairs for which the scheme gives a floor at all
        for (int a = 0; a < kNumAdapters; ++a) for (double thr : kThresholds) floors += score_floor((int)strlen(kAdapters[a]), thr, sc) > 0;
        printf("scheme %d,%d,%d,%d: cases=%ld kept=%ld realigned=%ld floors=%d below_floor=%ld bad=%ld\n", sc[0], sc[1], sc[2], sc[3], t.cases, t.kept,
               t.realigned, floors, t.below_floor, t.bad);
        // the rule neither keeps nothing nor everything: at least 25 % kept and 10 % realigned of the non-failed pairs
        if (judged == 0 || t.kept * 4 < judged || t.realigned * 10 < judged || (floors > 0 && t.below_floor == 0)) { ++bad; printf("BAD scheme %d: a one-sided test\n", si); }
        bad += t.bad;
        cases += t.cases;
    }
    printf("cases=%ld bad=%ld \n", cases, bad);
    return bad ? 1 : 0;
}
