// test_consensus_quality.cpp -- pcc's two vote margins (csrc/pc_consensus.h: column_margin, slot_margin, quality_index) against a
// naive restatement of the rule, on the host: every vector of five column counters in 0 .. 4 with every template code 0 .. 4 and
// both tmpl_counts, every four slot counters in 0 .. 3 with voters from their sum to their sum + 4, and hand-stated cases.  A
// stand-alone program; tests/test_consensus_quality_host.py builds it under ASan and UBSan and runs it.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "pc_consensus.h"

static long cases = 0, bad = 0;

#define EXPECT(cond)                                                                                          \
    do {                                                                                                      \
        ++cases;                                                                                              \
        if (!(cond)) { ++bad; if (bad <= 20) printf("FAILED line %d: %s\n", __LINE__, #cond); }                \
    } while (0)

// The rule as the issue states it, with vectors and std::max: e[k] = c[k] - 1 for the template's code when the template is an
// earlier consensus; margin = max(0, e[b] - max over k != b of e[k]).
static long naive_column(const uint32_t *c, int tmpl_code, int tmpl_counts, int b)
{
    std::vector<long> e(c, c + 5);
    if (tmpl_counts == 0 && tmpl_code < 4) e[tmpl_code] -= 1;
    std::vector<long> others;
    for (int k = 0; k < 5; ++k) if (k != b) others.push_back(e[k]);
    return std::max(0L, e[b] - *std::max_element(others.begin(), others.end()));
}

// absent = voters - sum(cnt); margin = max(0, cnt[b] - max(absent, max over k != b of cnt[k]))
static long naive_slot(const uint32_t *cnt, uint32_t voters, int b)
{
    long sum = 0;
    std::vector<long> others;
    for (int k = 0; k < 4; ++k) { sum += cnt[k]; if (k != b) others.push_back(cnt[k]); }
    const long absent = (long)voters - sum;
    return std::max(0L, (long)cnt[b] - std::max(absent, *std::max_element(others.begin(), others.end())));
}

int main()
{
    long columns = 0, slots = 0, emitted_slots = 0, seen_col[6] = {0, 0, 0, 0, 0, 0}, seen_slot[4] = {0, 0, 0, 0};
    // every five counters in 0 .. 4 as the members left them, every template code, both tmpl_counts; the call adds the template's
    // own vote first, and the margin is asked for the base the call emits (nothing when deletion leads)
    for (int word = 0; word < 5 * 5 * 5 * 5 * 5; ++word) {
        for (int tc = 0; tc <= 4; ++tc) {
            uint32_t c[5];
            for (int k = 0, w = word; k < 5; ++k, w /= 5) c[k] = (uint32_t)(w % 5);
            if (tc < 4) c[tc] += 1;
            const int b = pcc::call_column(c, tc);
            for (int b_any = 0; b_any < 4; ++b_any) {                   // the function itself, for every base, called or not
                for (int counts = 0; counts <= 1; ++counts) {
                    const long want = naive_column(c, tc, counts, b_any);
                    EXPECT((long)pcc::column_margin(c, tc, counts, b_any) == want);
                    if (b_any == b) { ++columns; seen_col[std::min(want, 5L)] += 1; }
                }
            }
            if (b < 4) {                                               // the emitted base leads: never negative before the clamp with tmpl_counts 1
                long rest = 0;
                for (int k = 0; k < 5; ++k) if (k != b) rest = std::max(rest, (long)c[k]);
                EXPECT((long)pcc::column_margin(c, tc, 1, b) == (long)c[b] - rest);
            }
        }
    }
    // every four slot counters in 0 .. 3, voters from their sum to their sum + 4, every base (and the one the call emits)
    for (int word = 0; word < 4 * 4 * 4 * 4; ++word) {
        uint32_t cnt[4];
        uint32_t sum = 0;
        for (int k = 0, w = word; k < 4; ++k, w /= 4) { cnt[k] = (uint32_t)(w % 4); sum += cnt[k]; }
        for (uint32_t voters = sum; voters <= sum + 4; ++voters) {
            const int b = pcc::call_slot(cnt, voters);
            for (int b_any = 0; b_any < 4; ++b_any) {
                const long want = naive_slot(cnt, voters, b_any);
                EXPECT((long)pcc::slot_margin(cnt, voters, b_any) == want);
                ++slots;
                if (b_any == b) { ++emitted_slots; seen_slot[std::min(want, 3L)] += 1; }
            }
        }
    }
    for (int m = 0; m <= 5; ++m) EXPECT(seen_col[m] > 0);
    for (int m = 0; m <= 3; ++m) EXPECT(seen_slot[m] > 0);

    // hand-stated.  {A, C, G, T, deletion}; the template's own vote is in the counters
    long hand = cases;
    { const uint32_t v[5] = {2, 0, 0, 3, 0};                            // members 2 : 2, the template's T decides the tie
      EXPECT(pcc::call_column(v, 3) == 3);
      EXPECT(pcc::column_margin(v, 3, 0, 3) == 0);                      // an earlier consensus is no evidence: 2 against 2
      EXPECT(pcc::column_margin(v, 3, 1, 3) == 1); }                    // a read of the group: 3 against 2
    { const uint32_t v[5] = {3, 0, 0, 1, 0};                            // outvoted 3 : 1
      EXPECT(pcc::column_margin(v, 3, 1, 0) == 2 && pcc::column_margin(v, 3, 0, 0) == 3); }
    { const uint32_t v[5] = {0, 0, 4, 0, 3};                            // deletion is one of the alternatives
      EXPECT(pcc::column_margin(v, 2, 1, 2) == 1 && pcc::column_margin(v, 2, 0, 2) == 0); }
    { const uint32_t v[5] = {0, 2, 0, 0, 0};                            // the template holds an N: nothing is taken off
      EXPECT(pcc::column_margin(v, 4, 0, 1) == 2 && pcc::column_margin(v, 4, 1, 1) == 2); }
    { const uint32_t v[5] = {1, 1, 0, 0, 0};                            // a lone template base against one member, as an earlier consensus
      EXPECT(pcc::call_column(v, 0) == 0 && pcc::column_margin(v, 0, 0, 0) == 0); }
    { const uint32_t v[4] = {0, 0, 0, 3}; EXPECT(pcc::slot_margin(v, 4, 3) == 2); }          // three of four hold it, one is absent
    { const uint32_t v[4] = {0, 0, 0, 3}; EXPECT(pcc::slot_margin(v, 5, 3) == 1); }
    { const uint32_t v[4] = {0, 3, 0, 2}; EXPECT(pcc::slot_margin(v, 9, 1) == 0); }          // the leader is below absent = 4
    { const uint32_t v[4] = {0, 3, 3, 0}; EXPECT(pcc::slot_margin(v, 6, 1) == 0); }          // a tie between two bases
    { const uint32_t v[4] = {5, 0, 0, 1}; EXPECT(pcc::slot_margin(v, 6, 0) == 4); }
    { const uint32_t v[5] = {301, 0, 0, 0, 1};                          // a margin of 300 indexes entry 255
      EXPECT(pcc::column_margin(v, 0, 1, 0) == 300 && pcc::quality_index(300) == 255); }
    EXPECT(pcc::quality_index(0) == 0 && pcc::quality_index(254) == 254 && pcc::quality_index(255) == 255 && pcc::quality_index(256) == 255);
    EXPECT(pcc::quality_index(0xffffffffu) == 255);
    { const uint32_t v[5] = {0xffffffffu, 0, 0, 0, 0}; EXPECT(pcc::column_margin(v, 0, 1, 0) == 0xffffffffu); }      // no overflow on the way
    { const uint32_t v[4] = {0xffffffffu, 0, 0, 0}; EXPECT(pcc::slot_margin(v, 0xffffffffu, 0) == 0xffffffffu); }
    EXPECT(pcc::QUAL_ENTRIES == 256 && pcc::MAX_QUAL == 93);
    hand = cases - hand;

    printf("cases=%ld bad=%ld columns=%ld slots=%ld emitted_slots=%ld hand=%ld\n", cases, bad, columns, slots, emitted_slots, hand);
    return bad ? 1 : 0;
}
