// The prefilter's table plan (porechop_amd/csrc/pc_prefilter_plan.h) for adapters with IUPAC letters, in both modes, printed
// for tests/test_wildcards_cpu.py to hold against the rule:
//   test_wildcards_plan ADAPTER MAX_EDITS [ADAPTER MAX_EDITS ...]
// per adapter (each planned alone), route (0 bytes, 1 plane seeds, 2 plane total) and mode (0 off, 1 on) one line
//   adapter route mode  pieces_seeded seeds_only  len  eq[0..4] of the first piece  then the exhaustive table's rows of slot 0:
//   256 words (routes 0, 1) or 4 words (route 2) of the first launch, all in hex
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pc_prefilter_plan.h"

int main(int argc, char **argv)
{
    for (int a = 1; a + 1 < argc; a += 2) {
        const std::vector<std::string> adapters{argv[a]};
        const int32_t ids[1] = {0}, ks[1] = {atoi(argv[a + 1])};
        for (int route = 0; route < 3; ++route)
            for (int mode = 0; mode < 2; ++mode) {
                pcp::Plan p;
                if (pcp::build(adapters, ids, ks, 1, (pcp::Route)route, pcp::Options(), p, mode != 0)) return 2;
                const int len = p.launches.empty() ? 0 : p.meta[p.launches[0].meta_off];
                const pcp::Piece pc{0, 0, len, ks[0], 0, 1u};
                uint32_t eq[5];
                pcp::eq_words(adapters[0], pc, eq, mode != 0);
                printf("%s %d %d %d %d %d", argv[a], route, mode, p.npieces, p.seeds_only ? 1 : 0, len);
                for (uint32_t e : eq) printf(" %08x", e);
                if (!p.launches.empty()) {
                    const pcp::Launch &L = p.launches[0];
                    const size_t rows = route == 2 ? 4 : 256;
                    for (size_t r = 0; r < rows; ++r) printf(" %08x", p.tables[L.table_off + r * L.P]);
                }
                printf("\n");
            }
    }
    return 0;
}
