// Host-side test of porechop_amd/csrc/pc_paths.h -- the plain-int32 alignment that hands back its PATH -- against the
// oracle (oracle/pc_oracle.c) on the case generator of tests/host/test_slow.cpp: unrestricted integer schemes, linear
// gaps, non-negative gaps, match <= mismatch, gap_open > gap_extend, letters N a c g t U - X.  The same align_path() the
// device runs per lane, with the device's nibble packing (eight rows to a dword) as the memory policy.
//
// Per case: (a) the digest is the oracle's; (b) the forward operations, replayed from (adapter_first, read_first), stay
// inside the rectangle with every '=' on equal and every 'X' on unequal Dna5 codes; (c) the replay ends in the last row
// or column, at the oracle's end cell; (d) head + path + tail is the oracle's path length; (e) the path starts in row 0
// or column 0; (f) the operations realise the score; (g) the digest recomputed from the gapped rows H^a V^b P H^c V^d by
// alignment.cpp's rule is the function's own; (h) the run-length formatter round-trips; (i) pcs::align_pair (pc_slow.h)
// gives the same eight digest fields, and align_path_window(n, m, 0, n, ...) called directly the same digest, head and
// operation words: the three routines over the one cell of pc_cell.h agree on every case.
//
//   g++ -O2 -std=c++17 -I porechop_amd/csrc -I oracle tests/host/test_paths.cpp oracle/pc_oracle.o
//   ./a.out [cases [seed [dump]]]
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "pc_paths.h"
#include "pc_slow.h"
extern "C" {
#include "pc_oracle.h"
}

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

struct SlowMem {                        // pc_slow.h's policy: one trace byte per cell
    std::vector<int> *m, *h; std::vector<uint8_t> *t; int rows;
    int &M(int i) { return (*m)[i]; }
    int &H(int i) { return (*h)[i]; }
    uint8_t &T(int j, int i) { return (*t).at((size_t)j * (rows + 1) + i); }
};

static bool same_digest(const pcw::Digest &a, const pcw::Digest &b)
{
    return a.read_start == b.read_start && a.read_end == b.read_end && a.adapter_start == b.adapter_start &&
           a.adapter_end == b.adapter_end && a.score == b.score && a.matches == b.matches && a.aligned_len == b.aligned_len &&
           a.full_len == b.full_len;
}

// alignment.cpp:6-111 over two gapped rows, as the oracle applies it (start / end = first / last column by which both rows
// have shown a base; identities over [start, end] and over the adapter's span)
struct RowDigest { int read_start, read_end, adapter_start, adapter_end, am, al, fm, fl, failed; };
static RowDigest digest_of_rows(const std::string &r0, const std::string &r1)
{
    RowDigest d = {-1, 0, -1, 0, 0, 0, 0, 0, 0};
    const int L = (int)r0.size();
    int start = -1, end = -1;
    bool rs = false, as = false;
    for (int i = 0; i < L; ++i) { rs |= r0[i] != '-'; as |= r1[i] != '-'; if (rs && as) { start = i; break; } }
    rs = as = false;
    for (int i = L - 1; i >= 0; --i) { rs |= r0[i] != '-'; as |= r1[i] != '-'; if (rs && as) { end = i; break; } }
    if (L == 0 || start < 0 || end < 0) { d.failed = 1; return d; }
    int aS = -1, aE = -1;
    for (int i = 0; i < L; ++i) if (r1[i] != '-') { aS = i; break; }
    for (int i = L - 1; i >= 0; --i) if (r1[i] != '-') { aE = i; break; }
    for (int i = start; i <= end; ++i) d.am += r0[i] == r1[i];
    for (int i = aS; i <= aE; ++i) d.fm += r0[i] == r1[i];
    d.al = end - start + 1; d.fl = aE - aS + 1;
    int rb = 0, ab = 0;
    for (int i = 0; i < L; ++i) {
        if (i == start) { d.read_start = rb; d.adapter_start = ab; }
        if (i == end) { d.read_end = rb; d.adapter_end = ab; }
        rb += r0[i] != '-'; ab += r1[i] != '-';
    }
    return d;
}

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 30000;
    std::mt19937_64 rng(argc > 2 ? atol(argv[2]) : 12345);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    long done = 0, bad = 0, one_cell = 0, linear = 0, posgap = 0, gapped = 0, empty_path = 0, open_above = 0, groups_seen[5] = {0, 0, 0, 0, 0};
    const bool dump = argc > 3;          // a third argument: one line per case for tests/pathcheck.py ('.' = empty string)
    const char *letters = "ACGTACGTACGTACGTNacgtU-X";
    static const char LET[5] = {'A', 'C', 'G', 'T', 'N'};
    while (done < cases) {
        int sc[4];
        const int mode = pick(0, 7);
        if (mode <= 1) for (int &x : sc) x = pick(-12, 12);
        else if (mode == 2) for (int &x : sc) x = pick(-100000, 100000);
        else if (mode == 3) { sc[0] = pick(1, 8); sc[1] = pick(-8, 0); sc[2] = pick(0, 6); sc[3] = pick(0, 6); }
        else if (mode == 4) for (int &x : sc) x = pick(-1, 1);
        else if (mode == 5) { sc[0] = pick(1, 6); sc[1] = pick(-8, -1); sc[2] = sc[3] = pick(-7, 2); }
        else if (mode == 6) { sc[0] = pick(1, 6); sc[1] = pick(-8, -1); sc[3] = pick(-9, -2); sc[2] = pick(sc[3] + 1, -1); }   // open > extend
        else { sc[0] = 3; sc[1] = -6; sc[2] = pick(0, 1) ? -2 : -5; sc[3] = sc[2] == -2 ? -5 : -2; }
        // test_slow.cpp's sets, and the adapter lengths at which a row group of the packed trace is partial, full or new
        const int nn[] = {0, 1, 3, 10, 40, 150, 300}, mm[] = {0, 1, 2, 5, 22, 28, 60, 130, 300, 7, 8, 9, 17};
        const int n = nn[pick(0, 6)], m = mm[pick(0, 12)];
        std::string rd(n, 'A'), ad(m, 'A');
        for (char &c : rd) c = letters[pick(0, 23)];
        if (n >= m && m > 0 && pick(0, 9) < 6) {
            const int s = pick(0, n - m);
            for (int k = 0; k < m; ++k) ad[k] = pick(0, 99) < 15 ? "ACGTN"[pick(0, 4)] : rd[s + k];
        } else for (char &c : ad) c = "ACGT"[pick(0, 3)];
        if (!pcs::fits(n, m, sc[0], sc[1], sc[2], sc[3])) continue;
        pc_oracle_result R;
        if (pc_oracle_align_raw(rd.c_str(), n, ad.c_str(), m, sc[0], sc[1], sc[2], sc[3], &R) != 0) continue;
        ++done;
        const int groups = pcpath::row_groups(m);
        std::vector<int> M(m + 1), H(m + 1);
        std::vector<uint32_t> T((size_t)(n + 1) * std::max(1, groups), 0xffffffffu);
        std::vector<uint32_t> ops((size_t)pcpath::ops_words(n, m) + 1, 0u);
        pcw::Digest d;
        int32_t head[4] = {-1, -1, -1, -1};
        int sink_bad = 0, next_word = 0;
        auto rdf = [&](int k) { return dna5((unsigned char)rd[k]); };
        auto adf = [&](int k) { return dna5((unsigned char)ad[k]); };
        const int err = pcpath::align_path(n, m, rdf, adf, sc[0], sc[1], sc[2], sc[3], Mem{&M, &H, &T, groups}, d, head,
                                           [&](int k, uint32_t w) {
                                               // dwords leave in order, each once, inside ceil((n + m) / 16)
                                               if (k != next_word || k >= pcpath::ops_words(n, m)) sink_bad = 1; else ops[k] = w;
                                               ++next_word;
                                           });
        // (i) the same pair through the other two entrances of the one cell
        const char *why_one = nullptr;
        {
            std::vector<int> M2(m + 1), H2(m + 1);
            std::vector<uint8_t> T2((size_t)(n + 1) * (m + 1), 0xff);
            pcw::Digest ds;
            if (pcs::align_pair(n, m, rdf, adf, sc[0], sc[1], sc[2], sc[3], SlowMem{&M2, &H2, &T2, m}, ds) != err || !same_digest(ds, d))
                why_one = "(i) pcs::align_pair != align_path";
            std::vector<uint32_t> T3(T.size(), 0xffffffffu), ops3(ops.size(), 0u);
            pcw::Digest dw;
            int32_t head3[4] = {-1, -1, -1, -1};
            const int errw = pcpath::align_path_window(n, m, 0, n, rdf, adf, sc[0], sc[1], sc[2], sc[3], Mem{&M2, &H2, &T3, groups}, dw,
                                                       head3, [&](int k, uint32_t w) { ops3.at(k) = w; });
            if (errw != err || !same_digest(dw, d) || memcmp(head3, head, sizeof head) || ops3 != ops)
                why_one = "(i) align_path_window(0, n) != align_path";
        }
        one_cell += why_one == nullptr;
        const bool lin = sc[2] == sc[3];
        linear += lin; posgap += sc[2] >= 0 || sc[3] >= 0; open_above += sc[2] > sc[3];
        const int watched[5] = {1, 7, 8, 9, 17};
        for (int q = 0; q < 5 && n > 0; ++q) groups_seen[q] += m == watched[q];
        if (dump) {
            std::string fwd;
            for (int k = head[0] - 1; k >= 0; --k) fwd += "=XID"[(ops[k / 16] >> (2 * (k % 16))) & 3u];
            printf("CASE %s %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n", n ? rd.c_str() : ".", m ? ad.c_str() : ".", sc[0], sc[1], sc[2],
                   sc[3], d.read_start, d.read_end, d.adapter_start, d.adapter_end, d.score, d.matches, d.aligned_len, d.full_len, head[0],
                   head[1], head[2], head[3], fwd.empty() ? "." : fwd.c_str());
        }
        const char *why = nullptr;
        // (a)
        bool same;
        if (R.failed) same = d.read_start == -1 && (n == 0 || m == 0 ? d.score == R.score : true);
        else same = d.read_start == R.read_start && d.read_end == R.read_end && d.adapter_start == R.adapter_start &&
                    d.adapter_end == R.adapter_end && d.score == R.score && d.matches == R.aligned_matches &&
                    d.matches == R.full_matches && d.aligned_len == R.aligned_len && d.full_len == R.full_len;
        if (err) why = "err";
        else if (why_one) why = why_one;
        else if (sink_bad) why = "sink order / bound";
        else if (!same) why = "(a) digest != oracle";
        else if (n == 0 || m == 0) {
            if (head[0] || head[1] || head[2] || head[3] || next_word != 0 || d.score != INT_MIN || d.read_end || d.adapter_start != -1 ||
                d.adapter_end || d.matches || d.aligned_len || d.full_len) why = "empty input: record / head";
        } else {
            const int L = head[0], a = head[1], b = head[2], opens = head[3];
            if (next_word != (L + 15) / 16) why = "dwords handed out";
            // forward operations
            std::string fwd(L, '?');
            for (int k = 0; k < L && !why; ++k) fwd[L - 1 - k] = "=XID"[(ops[k / 16] >> (2 * (k % 16))) & 3u];
            if (L % 16 && (ops[L / 16] >> (2 * (L % 16)))) why = "bits above the last operation";
            long cnt[4] = {0, 0, 0, 0};
            int i = b, j = a;
            std::string r0, r1;
            for (int k = 0; k < a; ++k) { r0 += LET[rdf(k)]; r1 += '-'; }
            for (int k = 0; k < b; ++k) { r0 += '-'; r1 += LET[adf(k)]; }
            for (int k = 0; k < L && !why; ++k) {
                const char op = fwd[k];
                if (op == '=' || op == 'X') {
                    if (i >= m || j >= n) { why = "(b) left the rectangle"; break; }
                    if ((rdf(j) == adf(i)) != (op == '=')) { why = "(b) = / X against the bases"; break; }
                    r0 += LET[rdf(j)]; r1 += LET[adf(i)];
                    ++i; ++j; ++cnt[op == '=' ? 0 : 1];
                } else if (op == 'I') {
                    if (j >= n) { why = "(b) left the rectangle"; break; }
                    r0 += LET[rdf(j)]; r1 += '-';
                    ++j; ++cnt[2];
                } else {
                    if (i >= m) { why = "(b) left the rectangle"; break; }
                    r0 += '-'; r1 += LET[adf(i)];
                    ++i; ++cnt[3];
                }
            }
            if (!why && !(i == m || j == n)) why = "(c) does not end in the last row or column";
            if (!why && (i != R.end_i || j != R.end_j)) why = "(c) end cell != oracle";
            if (!why && a + b + L + (n - R.end_j) + (m - R.end_i) != R.path_len) why = "(d) path length";
            if (!why && !(a == 0 || b == 0)) why = "(e) head";
            const long long ge = lin ? sc[2] : sc[3];
            if (!why && (long long)sc[0] * cnt[0] + (long long)sc[1] * cnt[1] + (long long)opens * sc[2] + (cnt[2] + cnt[3] - opens) * ge != d.score)
                why = "(f) score";
            if (!why) {
                for (int k = j; k < n; ++k) { r0 += LET[rdf(k)]; r1 += '-'; }
                for (int k = i; k < m; ++k) { r0 += '-'; r1 += LET[adf(k)]; }
                const RowDigest g = digest_of_rows(r0, r1);
                if (g.failed || g.read_start != d.read_start || g.read_end != d.read_end || g.adapter_start != d.adapter_start ||
                    g.adapter_end != d.adapter_end || g.am != d.matches || g.fm != d.matches || g.al != d.aligned_len || g.fl != d.full_len)
                    why = "(g) digest of the gapped rows";
            }
            if (!why) {
                // (h) the run-length string, sized by a first call, expands to the forward operations
                const int need = pcpath::path_cigar(ops.data(), L, nullptr, 0);
                std::vector<char> buf((size_t)need + 1, '#');
                const int need2 = pcpath::path_cigar(ops.data(), L, buf.data(), buf.size());
                std::string back;
                bool ok = need2 == need && buf[need] == '\0';
                long run = 0;
                char prev = 0;
                for (int k = 0; k < need && ok; ++k) {
                    const char ch = buf[k];
                    if (ch >= '0' && ch <= '9') run = run * 10 + (ch - '0');
                    else { ok = run > 0 && ch != prev && (ch == '=' || ch == 'X' || ch == 'I' || ch == 'D'); back.append((size_t)run, ch); prev = ch; run = 0; }
                }
                if (!ok || run != 0 || back != fwd) why = "(h) formatter";
                if (need > 2) {                                  // a short buffer: the same length, nothing written beyond it
                    char small[3] = {'#', '#', '#'};
                    if (pcpath::path_cigar(ops.data(), L, small, 2) != need || small[0] != buf[0] || small[1] != '\0' || small[2] != '#') why = "(h) short buffer";
                }
            }
            gapped += cnt[2] + cnt[3] > 0; empty_path += L == 0;
        }
        if (why && ++bad <= 10)
            printf("MISMATCH %s rd=%s ad=%s scores=%d,%d,%d,%d\n got  %d,%d,%d,%d,%d m=%d al=%d fl=%d head=%d,%d,%d,%d\n want %d,%d,%d,%d,%d m=%d/%d al=%d fl=%d failed=%d end=%d,%d len=%d\n",
                   why, rd.c_str(), ad.c_str(), sc[0], sc[1], sc[2], sc[3], d.read_start, d.read_end, d.adapter_start, d.adapter_end,
                   d.score, d.matches, d.aligned_len, d.full_len, head[0], head[1], head[2], head[3], R.read_start, R.read_end, R.adapter_start,
                   R.adapter_end, R.score, R.aligned_matches, R.full_matches, R.aligned_len, R.full_len, R.failed, R.end_i, R.end_j, R.path_len);
    }
    printf("cases=%ld bad=%ld one_cell=%ld linear=%ld nonnegative_gap=%ld open_above_extend=%ld gapped=%ld empty_path=%ld rows1=%ld rows7=%ld rows8=%ld rows9=%ld rows17=%ld\n",
           done, bad, one_cell, linear, posgap, open_above, gapped, empty_path, groups_seen[0], groups_seen[1], groups_seen[2], groups_seen[3], groups_seen[4]);
    return bad ? 1 : 0;
}
