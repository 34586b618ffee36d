// tests/host/test_umi_strands.cpp -- the both-strands rule on the host, stand-alone (built with ASan and UBSan by
// tests/test_umi_strands_host.py): pcud::mirror / mirror_composition of pc_umi_dist.h and pcc::comp_code / member_byte of
// pc_consensus.h.
//   1. pcud::mirror against a per-base loop for every length 0 .. 64 on seeded keys (garbage above the length), the result's
//      bits above the length 0, and mirror(mirror(k)) == k under the mask
//   2. mirror_composition(composition(k)) == composition(mirror(k)); the bound over (own composition, mirrored composition of
//      the other) never above the true d(a, mirror(b)), the plain DP over the reverse-complemented STRING, on argv[1] (default
//      20000) seeded pairs; and d(a, mirror(b)) == d(mirror(a), b)
//   3. pcc::comp_code on all 256 bytes against a table written out here
//   4. pcc::fill / walk / votes of a member handed over through pcc::member_byte(reverse) equal those of the reverse
//      complement materialised by this file's own string routine: N, lower case and U included
// The last line of the output holds the counters as name=value; bad=0 is a pass.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "pc_consensus.h"
#include "pc_umi_dist.h"

namespace {

std::mt19937_64 rng(20261022);

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

// the reverse complement of a string, letter by letter: upper case out, U as T, anything else N
std::string revcomp(const std::string &s)
{
    std::string r;
    for (size_t t = s.size(); t-- > 0;) {
        switch (s[t]) {
        case 'A': case 'a': r += 'T'; break;
        case 'C': case 'c': r += 'G'; break;
        case 'G': case 'g': r += 'C'; break;
        case 'T': case 't': case 'U': case 'u': r += 'A'; break;
        default: r += 'N';
        }
    }
    return r;
}

struct Counters {
    long bad = 0, mirrors = 0, pairs = 0, bound_ok = 0, bound_tight = 0, bound_binds = 0, planted = 0, codes = 0, pileups = 0, accepted = 0,
         with_n = 0;
} n;

void fail(const char *what, const std::string &a, const std::string &b)
{
    if (++n.bad <= 5) printf("MISMATCH %s a=%s b=%s\n", what, a.c_str(), b.c_str());
}

void check_mirror(const std::string &s)
{
    const int len = (int)s.size();
    const pcud::Key k = pack(s), m = pcud::mirror(k, len);
    ++n.mirrors;
    bool ok = (m.p0 & ~pcud::len_mask(len)) == 0 && (m.p1 & ~pcud::len_mask(len)) == 0;
    for (int t = 0; t < len; ++t) ok = ok && pcud::base_at(m, t) == 3 - pcud::base_at(k, len - 1 - t);
    const std::string rc = revcomp(s);
    for (int t = 0; t < len; ++t) ok = ok && pcud::base_at(m, t) == code_of(rc[t]);
    const pcud::Key back = pcud::mirror(m, len);
    ok = ok && back.p0 == (k.p0 & pcud::len_mask(len)) && back.p1 == (k.p1 & pcud::len_mask(len));
    ok = ok && pcud::mirror_composition(pcud::composition(k, len)) == pcud::composition(m, len);
    if (!ok) fail("mirror", s, rc);
}

void check_pair(const std::string &a, const std::string &b)
{
    const int la = (int)a.size(), lb = (int)b.size();
    const pcud::Key ka = pack(a), kb = pack(b);
    const int want = naive(a, revcomp(b));
    ++n.pairs;
    bool ok = pcud::distance_any(ka, la, pcud::mirror(kb, lb), lb) == want && pcud::distance_any(pcud::mirror(ka, la), la, kb, lb) == want;
    const int lo = pcud::lower_bound_packed(pcud::composition(ka, la), la, pcud::mirror_composition(pcud::composition(kb, lb)), lb);
    ok = ok && lo == pcud::lower_bound(ka, la, pcud::mirror(kb, lb), lb) && lo <= want;
    if (lo <= want) ++n.bound_ok;
    if (lo == want && want > 0) ++n.bound_tight;
    if (lo > 2) ++n.bound_binds;
    if (!ok) fail("pair", a, b);
}

std::vector<uint32_t> pile(const std::string &tmpl, const std::vector<uint8_t> &member, int band, int32_t &d)
{
    const int la = (int)tmpl.size(), lb = (int)member.size();
    std::vector<int32_t> row((size_t)pcc::width(band));
    std::vector<uint8_t> trace((size_t)pcc::trace_bytes(la));
    std::vector<uint32_t> votes((size_t)pcc::votes_per_group(la), 0);
    d = pcc::fill((const uint8_t *)tmpl.data(), la, member.data(), lb, band, row.data(), trace.data());
    if (!pcc::rejected(d, la, lb, 30)) {
        ++n.accepted;
        pcc::PtrSeq seq{member.data()};
        pcc::PtrTrace tr{trace.data()};
        struct Adder { uint32_t *v; void operator()(int64_t c) const { v[c] += 1; } } add{votes.data()};
        if (!pcc::walk(seq, la, lb, band, tr, add)) votes.assign(votes.size(), 0xffffffffu);
    }
    return votes;
}

void check_pileup(const std::string &tmpl, const std::string &stored, int band)
{
    const int lb = (int)stored.size();
    std::vector<uint8_t> through((size_t)lb), plain((size_t)lb);
    for (int j = 0; j < lb; ++j) {
        through[(size_t)j] = pcc::member_byte((const uint8_t *)stored.data(), lb, j, true);
        plain[(size_t)j] = pcc::member_byte((const uint8_t *)stored.data(), lb, j, false);
    }
    const std::string rc = revcomp(stored);
    const std::vector<uint8_t> want(rc.begin(), rc.end());
    ++n.pileups;
    bool ok = plain == std::vector<uint8_t>(stored.begin(), stored.end());
    for (int j = 0; j < lb; ++j) ok = ok && pcc::code(through[(size_t)j]) == pcc::code(want[(size_t)j]);
    int32_t d1 = 0, d2 = 0;
    const std::vector<uint32_t> v1 = pile(tmpl, through, band, d1), v2 = pile(tmpl, want, band, d2);
    ok = ok && d1 == d2 && v1 == v2;
    if (!ok) fail("pileup", tmpl, stored);
}

}  // namespace

int main(int argc, char **argv)
{
    const long seeded = argc > 1 ? atol(argv[1]) : 20000;
    // 1. mirrors at every length
    for (int len = 0; len <= 64; ++len)
        for (int k = 0; k < 40; ++k) check_mirror(random_string(len));
    check_mirror("ACGT");                                            // a self-mirror key
    // 2. the bound under the mirror
    static const int LENGTHS[] = {0, 1, 22, 31, 32, 33, 44, 63, 64};
    for (long k = 0; k < seeded; ++k) {
        const std::string a = random_string(LENGTHS[rng() % 9]);
        if (k & 1) { check_pair(a, revcomp(mutate(a, (int)(rng() % 7)))); ++n.planted; }     // b's mirror is a mutated a
        else check_pair(a, random_string(LENGTHS[rng() % 9]));
    }
    // 3. comp_code on every byte
    for (int b = 0; b < 256; ++b) {
        int want = 4;
        switch (b) {
        case 'A': case 'a': want = 3; break;
        case 'C': case 'c': want = 2; break;
        case 'G': case 'g': want = 1; break;
        case 'T': case 't': case 'U': case 'u': want = 0; break;
        }
        ++n.codes;
        if (pcc::comp_code(pcc::code((uint8_t)b)) != want || pcc::code(pcc::comp_letter((uint8_t)b)) != want) fail("comp_code", std::to_string(b), "");
    }
    for (int c = 0; c <= 4; ++c)
        if (pcc::comp_code(pcc::comp_code(c)) != c) fail("comp_code twice", std::to_string(c), "");
    // 4. pile-ups of members handed over reverse-complemented
    for (int k = 0; k < 400; ++k) {
        const int la = 1 + (int)(rng() % 300), band = 1 + (int)(rng() % pcc::MAX_BAND);
        std::string tmpl(la, 'A');
        for (char &ch : tmpl) ch = "ACGT"[rng() & 3];
        std::string member = tmpl;                                   // a mutated copy of the template ...
        const int edits = (int)(rng() % (1 + la / 8));
        for (int e = 0; e < edits; ++e) {
            const int kind = (int)(rng() % 3);
            if (kind == 0 && !member.empty()) member[rng() % member.size()] = "ACGT"[rng() & 3];
            else if (kind == 1) member.insert(member.begin() + rng() % (member.size() + 1), "ACGT"[rng() & 3]);
            else if (!member.empty()) member.erase(member.begin() + rng() % member.size());
        }
        std::string stored = revcomp(member);                        // ... stored as its reverse complement
        if (k % 3 == 0 && !stored.empty()) {
            ++n.with_n;
            for (int e = 0; e < 3; ++e) {
                char &ch = stored[rng() % stored.size()];
                const int kind = (int)(rng() % 3);
                ch = kind == 0 ? 'N' : (kind == 1 ? (char)(ch | 0x20) : (ch == 'T' ? 'U' : ch));
            }
        }
        check_pileup(tmpl, stored, band);
    }
    check_pileup("A", "", 1);
    check_pileup("ACGT", "ACGU", 2);
    printf("bad=%ld mirrors=%ld pairs=%ld bound_ok=%ld bound_tight=%ld bound_binds=%ld planted=%ld codes=%ld pileups=%ld accepted=%ld with_n=%ld\n",
           n.bad, n.mirrors, n.pairs, n.bound_ok, n.bound_tight, n.bound_binds, n.planted, n.codes, n.pileups, n.accepted, n.with_n);
    return n.bad == 0 ? 0 : 1;
}
