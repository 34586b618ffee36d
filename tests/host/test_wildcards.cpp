// Host-side test of the two plain-int32 routines with the adapter given as SETS (pc_letters.h): pcs::align_pair_sets
// (pc_slow.h) and pcpath::align_path_window_sets (pc_paths.h), the very functions the device runs per lane for a context with
// IUPAC wildcards, against cases dumped from tests/wild_ref.py -- the independent restatement of the rule.
//
// Input (argv[1]), one case per line, '.' for an empty string:
//   read adapter match mismatch gap_open gap_extend wildcards  rs re as ae score matches aligned_len full_len  read_first adapter_first cigar
// Per case: both routines give wild_ref's eight integers; the path's head and its run-length string are wild_ref's; and
// pcl::letter_set in the OTHER mode is exercised by the cases with wildcards = 0 (the reference's equality, N == N).
//
//   g++ -O2 -std=c++17 -I porechop_amd/csrc tests/host/test_wildcards.cpp && ./a.out cases.txt
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pc_paths.h"
#include "pc_slow.h"

struct Mem {
    std::vector<int> *m, *h; std::vector<uint32_t> *t; int groups;
    int &M(int i) { return (*m).at(i); }
    int &H(int i) { return (*h).at(i); }
    void put(int j, int g, uint32_t w) { (*t).at((size_t)j * groups + g) = w; }
    uint32_t get(int j, int g) { return (*t).at((size_t)j * groups + g); }
};

struct SlowMem {
    std::vector<int> *m, *h; std::vector<uint8_t> *t; int rows;
    int &M(int i) { return (*m).at(i); }
    int &H(int i) { return (*h).at(i); }
    uint8_t &T(int j, int i) { return (*t).at((size_t)j * (rows + 1) + i); }
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    long cases = 0, bad = 0, wild = 0, degenerate = 0, gapped = 0, linear = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string rd, ad, cigar;
        int sc[4], wc, want[8], rf, af;
        ls >> rd >> ad >> sc[0] >> sc[1] >> sc[2] >> sc[3] >> wc;
        for (int &x : want) ls >> x;
        ls >> rf >> af >> cigar;
        if (!ls) { fprintf(stderr, "unreadable case: %s\n", line.c_str()); return 2; }
        if (rd == ".") rd.clear();
        if (ad == ".") ad.clear();
        if (cigar == ".") cigar.clear();
        const int n = (int)rd.size(), m = (int)ad.size();
        ++cases;
        wild += wc != 0;
        linear += sc[2] == sc[3];
        for (char ch : ad) if (wc && pcl::degenerate((uint8_t)ch)) { ++degenerate; break; }
        auto rdf = [&](int k) { return pcc::dna5_code((uint8_t)rd.at(k)); };
        auto adf = [&](int k) { return pcl::letter_set((uint8_t)ad.at(k), wc != 0); };
        std::vector<int> M(m + 1), H(m + 1);

        pcw::Digest ds;
        std::vector<uint8_t> T8((size_t)(n + 1) * (m + 1), 0xff);
        int err = pcs::align_pair_sets(n, m, rdf, adf, sc[0], sc[1], sc[2], sc[3], SlowMem{&M, &H, &T8, m}, ds);

        const int groups = pcpath::row_groups(m);
        std::vector<uint32_t> T((size_t)(n + 1) * std::max(1, groups), 0xffffffffu);
        std::vector<uint32_t> ops((size_t)pcpath::ops_words(n, m) + 1, 0u);
        pcw::Digest dp;
        int32_t head[4];
        err |= pcpath::align_path_window_sets(n, m, 0, n, rdf, adf, sc[0], sc[1], sc[2], sc[3], Mem{&M, &H, &T, std::max(1, groups)}, dp,
                                              head, [&](int k, uint32_t w) { ops.at(k) = w; });
        const int got_s[8] = {ds.read_start, ds.read_end, ds.adapter_start, ds.adapter_end, ds.score, ds.matches, ds.aligned_len, ds.full_len};
        const int got_p[8] = {dp.read_start, dp.read_end, dp.adapter_start, dp.adapter_end, dp.score, dp.matches, dp.aligned_len, dp.full_len};
        bool ok = err == 0;
        // a failed alignment defines field 0 and the score only (alignment.cpp:9-21)
        const int fields = want[0] == -1 ? 1 : 8;
        for (int k = 0; k < fields; ++k) ok &= got_s[k] == want[k] && got_p[k] == want[k];
        ok &= got_s[4] == want[4] && got_p[4] == want[4];
        char buf[4096];
        pcpath::path_cigar(ops.data(), head[0], buf, sizeof buf);
        ok &= cigar == buf && head[1] == rf && head[2] == af;
        gapped += cigar.find('I') != std::string::npos || cigar.find('D') != std::string::npos;
        if (!ok && bad++ < 10)
            fprintf(stderr, "MISMATCH %s %s [%d %d %d %d] wc=%d: slow %d,%d,%d,%d,%d,%d,%d,%d path %d,%d,%d,%d,%d,%d,%d,%d head %d|%d|%s want %d,%d,%d,%d,%d,%d,%d,%d %d|%d|%s\n",
                    rd.c_str(), ad.c_str(), sc[0], sc[1], sc[2], sc[3], wc, got_s[0], got_s[1], got_s[2], got_s[3], got_s[4], got_s[5], got_s[6],
                    got_s[7], got_p[0], got_p[1], got_p[2], got_p[3], got_p[4], got_p[5], got_p[6], got_p[7], head[1], head[2], buf, want[0],
                    want[1], want[2], want[3], want[4], want[5], want[6], want[7], rf, af, cigar.c_str());
    }
    printf("cases=%ld bad=%ld wildcards=%ld degenerate=%ld gapped=%ld linear=%ld \n", cases, bad, wild, degenerate, gapped, linear);
    return bad ? 1 : 0;
}
