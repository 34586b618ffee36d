// tests/host/test_umi_dist.cpp -- pc_umi_dist.h on the host, stand-alone (built with ASan and UBSan by tests/test_umi_dist_host.py):
// pcud::distance at both widths against the plain DP, pcud::lower_bound against the distance.
//   1. every pair of strings over ACGT of length 0 .. 5
//   2. argv[1] (default 20000) seeded pairs, random and mutated, lengths drawn from {0, 1, 22, 31, 32, 33, 44, 63, 64}
// Every key carries garbage in its plane bits at and above its length.
// The last line of the output holds the counters as name=value; bad=0 is a pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "pc_umi_dist.h"

namespace {

std::mt19937_64 rng(20261021);

int code_of(char ch)
{
    switch (ch) { case 'A': return 0; case 'C': return 1; case 'G': return 2; default: return 3; }
}

pcud::Key pack(const std::string &s)
{
    pcud::Key k = {0, 0};
    for (size_t t = 0; t < s.size(); ++t) {
        const int c = code_of(s[t]);
        k.p0 |= (uint64_t)(c & 1) << t;
        k.p1 |= (uint64_t)(c >> 1) << t;
    }
    const uint64_t above = ~pcud::len_mask((int)s.size());
    k.p0 |= rng() & above;
    k.p1 |= rng() & above;
    return k;
}

int naive(const std::string &a, const std::string &b)
{
    std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int)j;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int)i;
        for (size_t j = 1; j <= b.size(); ++j)
            cur[j] = std::min({prev[j - 1] + (a[i - 1] != b[j - 1] ? 1 : 0), prev[j] + 1, cur[j - 1] + 1});
        std::swap(prev, cur);
    }
    return prev[b.size()];
}

std::string random_string(int n)
{
    std::string s(n, 'A');
    for (char &ch : s) ch = "ACGT"[rng() & 3];
    return s;
}

std::string mutate(std::string s, int edits)
{
    for (int e = 0; e < edits; ++e) {
        const int kind = (int)(rng() % 3);
        if (kind == 0 && !s.empty()) s[rng() % s.size()] = "ACGT"[rng() & 3];
        else if (kind == 1 && s.size() < 64) s.insert(s.begin() + rng() % (s.size() + 1), "ACGT"[rng() & 3]);
        else if (!s.empty()) s.erase(s.begin() + rng() % s.size());
    }
    return s;
}

struct Counters {
    long cases = 0, bad = 0, narrow = 0, wide = 0, bound_ok = 0, bind_len = 0, bind_plus = 0, bind_minus = 0, tight = 0, slack = 0,
         empty = 0, full64 = 0, mutated = 0, random = 0, exhaustive = 0;
} n;

void check(const std::string &a, const std::string &b)
{
    const int la = (int)a.size(), lb = (int)b.size();
    const pcud::Key ka = pack(a), kb = pack(b);
    const int want = naive(a, b);
    ++n.cases;
    bool ok = true;
    if (la <= 32 && lb <= 32) { ++n.narrow; ok = ok && pcud::distance<uint32_t>(ka, la, kb, lb) == want; }
    ++n.wide;
    ok = ok && pcud::distance<uint64_t>(ka, la, kb, lb) == want && pcud::distance_any(ka, la, kb, lb) == want;
    ok = ok && pcud::distance<uint64_t>(kb, lb, ka, la) == want;
    int t[3];
    pcud::lower_bound_terms(ka, la, kb, lb, t);
    const int lo = pcud::lower_bound(ka, la, kb, lb);
    ok = ok && lo == std::max({t[0], t[1], t[2]}) && lo <= want;
    ok = ok && lo == pcud::lower_bound_packed(pcud::composition(ka, la), la, pcud::composition(kb, lb), lb);
    if (lo <= want) ++n.bound_ok;
    if (t[0] == lo && t[0] > 0) ++n.bind_len;
    if (t[1] == lo && t[1] > t[2]) ++n.bind_plus;
    if (t[2] == lo && t[2] > t[1]) ++n.bind_minus;
    if (lo == want && want > 0) ++n.tight;
    if (lo < want) ++n.slack;
    if (la == 0 || lb == 0) ++n.empty;
    if (la == 64 && lb == 64) ++n.full64;
    if (!ok) {
        if (++n.bad <= 5) printf("MISMATCH a=%s b=%s want=%d wide=%d bound=%d\n", a.c_str(), b.c_str(), want,
                                 pcud::distance<uint64_t>(ka, la, kb, lb), lo);
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const long seeded = argc > 1 ? atol(argv[1]) : 20000;
    std::vector<std::string> all;
    for (int len = 0; len <= 5; ++len)
        for (int v = 0; v < (1 << (2 * len)); ++v) {
            std::string s(len, 'A');
            for (int t = 0; t < len; ++t) s[t] = "ACGT"[(v >> (2 * t)) & 3];
            all.push_back(s);
        }
    for (const std::string &a : all)
        for (const std::string &b : all) { check(a, b); ++n.exhaustive; }
    static const int LENGTHS[] = {0, 1, 22, 31, 32, 33, 44, 63, 64};
    for (long k = 0; k < seeded; ++k) {
        const std::string a = random_string(LENGTHS[rng() % 9]);
        if (k & 1) { check(a, mutate(a, (int)(rng() % 7))); ++n.mutated; }
        else { check(a, random_string(LENGTHS[rng() % 9])); ++n.random; }
    }
    printf("cases=%ld bad=%ld narrow=%ld wide=%ld bound_ok=%ld bind_len=%ld bind_plus=%ld bind_minus=%ld tight=%ld slack=%ld empty=%ld "
           "full64=%ld mutated=%ld random=%ld exhaustive=%ld\n",
           n.cases, n.bad, n.narrow, n.wide, n.bound_ok, n.bind_len, n.bind_plus, n.bind_minus, n.tight, n.slack, n.empty, n.full64,
           n.mutated, n.random, n.exhaustive);
    return n.bad == 0 ? 0 : 1;
}
