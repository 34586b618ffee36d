// Host test of porechop_amd/csrc/pc_consensus.h (namespace pcc): the banded alignment, its traceback and its votes against a
// naive full-matrix implementation written from the rule's text, and the call rule on hand-stated counters.
//   * every pair of strings over {A, C} of length 0 .. 4 (template length >= 1) at band 1, 2 and 8;
//   * argv[1] (default 5000) seeded mutated pairs of lengths 1 .. 300 at band 1 .. 64, some with N's and lower case, and a
//     fifth as many at band 65 .. 127;
//   * the banded distance equals the plain edit distance whenever band >= max(la, lb), and is never below it.
// Prints one line of counters; exit status 1 when anything differs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pc_consensus.h"

namespace {

const int64_t BIG = 1000000000;

int code_of(char ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    }
    return 4;
}

bool inside(int64_t i, int64_t j, int64_t la, int64_t lb, int band)
{
    const int64_t centre = i * lb / la;
    return std::llabs(j - centre) <= band;
}

// the whole (la + 1) x (lb + 1) matrix, cells outside the band BIG
std::vector<std::vector<int64_t>> matrix(const std::string &a, const std::string &b, int band, bool banded)
{
    const int la = (int)a.size(), lb = (int)b.size();
    std::vector<std::vector<int64_t>> D(la + 1, std::vector<int64_t>(lb + 1, BIG));
    for (int i = 0; i <= la; ++i)
        for (int j = 0; j <= lb; ++j) {
            if (banded && !inside(i, j, la, lb, band)) continue;
            if (i == 0 && j == 0) { D[i][j] = 0; continue; }
            int64_t v = BIG;
            if (i > 0 && j > 0) {
                const int ca = code_of(a[i - 1]), cb = code_of(b[j - 1]);
                v = std::min(v, D[i - 1][j - 1] + ((ca == cb && ca < 4) ? 0 : 1));
            }
            if (i > 0) v = std::min(v, D[i - 1][j] + 1);
            if (j > 0) v = std::min(v, D[i][j - 1] + 1);
            D[i][j] = std::min(v, BIG);
        }
    return D;
}

// the votes of the path the stated order picks, from the full matrix
std::vector<uint32_t> naive_votes(const std::string &a, const std::string &b, const std::vector<std::vector<int64_t>> &D)
{
    const int la = (int)a.size();
    std::vector<uint32_t> votes((size_t)(21 * la + 16), 0);
    int i = la, j = (int)b.size();
    std::vector<std::vector<int>> inserted(la + 1);                    // per gap, the member's inserted bases, last first
    while (i > 0 || j > 0) {
        const int64_t v = D[i][j];
        bool diag = false, del = false;
        if (i > 0 && j > 0) {
            const int ca = code_of(a[i - 1]), cb = code_of(b[j - 1]);
            diag = D[i - 1][j - 1] + ((ca == cb && ca < 4) ? 0 : 1) == v && D[i - 1][j - 1] < BIG;
        }
        if (!diag && i > 0) del = D[i - 1][j] + 1 == v && D[i - 1][j] < BIG;
        if (diag) {
            const int cb = code_of(b[j - 1]);
            if (cb < 4) votes[5 * (i - 1) + cb] += 1;
            --i; --j;
        } else if (del) {
            votes[5 * (i - 1) + 4] += 1;
            --i;
        } else {
            inserted[i].push_back(code_of(b[j - 1]));
            --j;
        }
    }
    for (int g = 0; g <= la; ++g) {
        std::reverse(inserted[g].begin(), inserted[g].end());
        for (int s = 0; s < (int)inserted[g].size() && s < PCC_INS_SLOTS; ++s)
            if (inserted[g][s] < 4) votes[5 * la + (g * PCC_INS_SLOTS + s) * 4 + inserted[g][s]] += 1;
    }
    return votes;
}

struct Adder {
    std::vector<uint32_t> *v;
    void operator()(int64_t counter) { (*v)[(size_t)counter] += 1; }
};

long cases = 0, bad = 0, exhaustive = 0, mutated = 0, wide = 0, above = 0, equal_narrow = 0, infinite = 0, with_ins = 0, with_del = 0,
     with_n = 0, rejected = 0, accepted = 0, broad = 0;

void check(const std::string &a, const std::string &b, int band)
{
    const int la = (int)a.size(), lb = (int)b.size();
    ++cases;
    const auto full = matrix(a, b, band, false), banded = matrix(a, b, band, true);
    const int64_t plain = full[la][lb], want = banded[la][lb];
    std::vector<int32_t> row((size_t)pcc::width(band));
    std::vector<uint8_t> trace((size_t)pcc::trace_bytes(la), 0xff);
    const int32_t got = pcc::fill((const uint8_t *)a.data(), la, (const uint8_t *)b.data(), lb, band, row.data(), trace.data());
    if (want >= BIG) {
        ++infinite;
        if (got != pcc::INF) { ++bad; printf("INF expected: a=%s b=%s band=%d got=%d\n", a.c_str(), b.c_str(), band, got); }
        return;
    }
    if (got != want) { ++bad; printf("distance: a=%s b=%s band=%d got=%d want=%lld\n", a.c_str(), b.c_str(), band, got, (long long)want); return; }
    if (want < plain) { ++bad; printf("below the plain distance: a=%s b=%s band=%d\n", a.c_str(), b.c_str(), band); }
    if (band >= std::max(la, lb)) {
        ++wide;
        if (want != plain) { ++bad; printf("wide band differs from the plain distance: a=%s b=%s band=%d\n", a.c_str(), b.c_str(), band); }
    } else if (want > plain) ++above;
    else ++equal_narrow;
    // the limit on either side of the rejection: d * 100 > pct * max(la, lb)
    const int64_t longest = std::max(la, lb);
    for (int pct = 0; pct <= 100; pct += 10) {
        const bool r = pcc::rejected(got, la, lb, pct);
        if (r != (want * 100 > (int64_t)pct * longest)) { ++bad; printf("rejected(): a=%s b=%s pct=%d\n", a.c_str(), b.c_str(), pct); }
        r ? ++rejected : ++accepted;
    }
    std::vector<uint32_t> votes((size_t)pcc::votes_per_group(la), 0);
    Adder add{&votes};
    pcc::PtrSeq seq{(const uint8_t *)b.data()};
    pcc::PtrTrace tr{trace.data()};
    if (!pcc::walk(seq, la, lb, band, tr, add)) { ++bad; printf("walk failed: a=%s b=%s band=%d\n", a.c_str(), b.c_str(), band); return; }
    const auto expect = naive_votes(a, b, banded);
    if (votes != expect) { ++bad; printf("votes: a=%s b=%s band=%d\n", a.c_str(), b.c_str(), band); }
    for (int i = 0; i < la; ++i) if (expect[5 * i + 4]) { ++with_del; break; }
    for (size_t t = 5 * (size_t)la; t < expect.size(); ++t) if (expect[t]) { ++with_ins; break; }
    if (b.find('N') != std::string::npos) ++with_n;
}

uint64_t state = 88172645463325252ull;
uint32_t rnd(uint32_t n)
{
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}

std::string mutate(const std::string &s, int per_mille)
{
    std::string out;
    for (char ch : s) {
        const uint32_t roll = rnd(1000);
        if (roll < (uint32_t)per_mille) continue;                                        // deleted
        if (roll < 2u * per_mille) { out.push_back("ACGT"[rnd(4)]); continue; }          // substituted
        if (roll < 3u * per_mille) out.push_back("ACGT"[rnd(4)]);                        // inserted before
        if (roll < 3u * per_mille + 20) { out.push_back(rnd(2) ? 'N' : (char)(ch | 0x20)); continue; }
        out.push_back(ch);
    }
    return out;
}

#define EXPECT(x) do { if (!(x)) { ++bad; printf("call rule: %s\n", #x); } ++calls; } while (0)

}  // namespace

int main(int argc, char **argv)
{
    const long n_mutated = argc > 1 ? atol(argv[1]) : 5000;
    // every pair over {A, C} of length 0 .. 4 (the template needs one base)
    std::vector<std::string> all = {""};
    for (size_t from = 0, len = 1; len <= 4; ++len) {
        const size_t to = all.size();
        for (size_t t = from; t < to; ++t) { all.push_back(all[t] + "A"); all.push_back(all[t] + "C"); }
        from = to;
    }
    for (const std::string &a : all) {
        if (a.empty()) continue;
        for (const std::string &b : all)
            for (int band : {1, 2, 8}) { check(a, b, band); ++exhaustive; }
    }
    for (long t = 0; t < n_mutated; ++t) {
        const int la = 1 + (int)rnd(300), band = 1 + (int)rnd(64);
        std::string a;
        for (int i = 0; i < la; ++i) a.push_back("ACGT"[rnd(4)]);
        std::string b = mutate(a, 10 + (int)rnd(120));
        if (rnd(8) == 0) b = b.substr(0, rnd((uint32_t)b.size() + 1));                    // a member much shorter than its template
        if (rnd(8) == 0) b += mutate(a, 50);                                             // and one about twice as long
        if (b.size() > 300) b.resize(300);
        check(a, b, band);
        ++mutated;
    }
    // and a fifth as many at band 65 .. 127, where a lane of the device holds three and four cells of a row
    for (long t = 0; t < n_mutated / 5; ++t) {
        const int la = 1 + (int)rnd(300), band = 65 + (int)rnd(63);
        std::string a;
        for (int i = 0; i < la; ++i) a.push_back("ACGT"[rnd(4)]);
        std::string b = mutate(a, 10 + (int)rnd(120));
        if (rnd(4) == 0) b += mutate(a, 50);
        if (b.size() > 400) b.resize(400);
        check(a, b, band);
        ++broad;
    }

    // the call rule on hand-stated counters: {A, C, G, T, deletion}
    long calls = 0;
    { const uint32_t v[5] = {1, 5, 2, 0, 3}; EXPECT(pcc::call_column(v, 0) == 1); }                  // a clear leader, not the template's base
    { const uint32_t v[5] = {1, 2, 2, 0, 6}; EXPECT(pcc::call_column(v, 1) == 4); }                  // deletion leads: nothing
    { const uint32_t v[5] = {0, 3, 3, 0, 1}; EXPECT(pcc::call_column(v, 2) == 2); }                  // tie, the template's base among the leaders
    { const uint32_t v[5] = {0, 3, 3, 0, 1}; EXPECT(pcc::call_column(v, 0) == 1); }                  // tie, the template's base not among them: smallest
    { const uint32_t v[5] = {0, 3, 3, 0, 1}; EXPECT(pcc::call_column(v, 4) == 1); }                  // the template holds an N: smallest
    { const uint32_t v[5] = {0, 0, 0, 4, 4}; EXPECT(pcc::call_column(v, 3) == 3); }                  // tie with deletion, the template's base wins
    { const uint32_t v[5] = {0, 0, 0, 4, 4}; EXPECT(pcc::call_column(v, 0) == 3); }                  // tie with deletion, a base is smaller than deletion
    { const uint32_t v[5] = {0, 0, 0, 0, 0}; EXPECT(pcc::call_column(v, 4) == 0); }                  // nobody voted
    { const uint32_t v[4] = {0, 2, 1, 0}; EXPECT(pcc::call_slot(v, 6) == -1); }                      // exactly half the voters: not emitted
    { const uint32_t v[4] = {0, 2, 2, 0}; EXPECT(pcc::call_slot(v, 6) == 1); }                       // more than half, tie to the smallest code
    { const uint32_t v[4] = {0, 1, 0, 3}; EXPECT(pcc::call_slot(v, 7) == 3); }
    { const uint32_t v[4] = {0, 0, 0, 0}; EXPECT(pcc::call_slot(v, 0) == -1); }
    EXPECT(pcc::code('a') == 0 && pcc::code('C') == 1 && pcc::code('g') == 2 && pcc::code('U') == 3 && pcc::code('t') == 3);
    EXPECT(pcc::code('N') == 4 && pcc::code('-') == 4 && pcc::code(0) == 4 && pcc::code('!') == 4 && pcc::code(0x81) == 4);

    printf("cases=%ld bad=%ld exhaustive=%ld mutated=%ld wide=%ld above=%ld equal_narrow=%ld infinite=%ld with_ins=%ld with_del=%ld with_n=%ld "
           "rejected=%ld accepted=%ld broad=%ld calls=%ld\n",
           cases, bad, exhaustive, mutated, wide, above, equal_narrow, infinite, with_ins, with_del, with_n, rejected, accepted, broad, calls);
    return bad ? 1 : 0;
}
