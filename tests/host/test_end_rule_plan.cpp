// Host check of the launch-plan decisions of a scan with an end rule (porechop_amd/csrc/pc_scan_plan.h): when short windows
// go through two passes, what the two-pass groups then carry for the rule, and which groups take the route.
#include <stdio.h>

#include <vector>

#include "pc_scan_plan.h"

static int bad = 0;
#define CHECK(x) do { if (!(x)) { ++bad; printf("BAD line %d: %s\n", __LINE__, #x); } } while (0)

int main()
{
    const int len[5] = {28, 33, 22, 30, 24}, window[5] = {100, 110, 90, 104, 94};
    const char slow[5] = {0, 0, 0, 0, 0};
    const pcn::Panel panel{5, len, window, slow};
    // the two-pass rule admits short windows under PC_MODE_AUTO with a rule, and only then
    CHECK(!pcn::two_pass_rule(PC_MODE_AUTO, 150, 100));
    CHECK(pcn::two_pass_rule(PC_MODE_AUTO, 150, 100, true));
    CHECK(pcn::two_pass_rule(PC_MODE_AUTO, 265, 100) && !pcn::two_pass_rule(PC_MODE_AUTO, 264, 100));
    CHECK(!pcn::two_pass_rule(PC_MODE_TRACE, 150, 100, true));

    // phase B of the headline: four jobs alone, start windows [0, 1000), end windows [1000, 2000)
    const int32_t adapter[4] = {0, 1, 2, 3};
    const int64_t start[5] = {0, 1000, 2000, 3000, 4000};
    const int32_t side[4] = {0, 0, 1, 1}, no_side[4] = {-1, -1, -1, -1};
    pcn::Params p;
    pcn::Table plain, ruled;
    CHECK(pcn::build_table(panel, p, adapter, nullptr, start, 4, 150, PC_MODE_AUTO, plain) == PC_OK);
    p.end_rule = true;
    CHECK(pcn::build_table(panel, p, adapter, nullptr, start, 4, 150, PC_MODE_AUTO, ruled) == PC_OK);
    // (the small single-pass groups of the call without a rule are merged; two-pass groups never are: one per row class)
    CHECK(plain.total == 4000 && ruled.total == 4000 && !plain.groups.empty() && ruled.groups.size() == 4);
    pcn::Floors f;
    f.rule_side = side;
    for (const pcn::Group &g : plain.groups) {
        CHECK(!g.two_pass);
        CHECK(!pcn::ruled(p, g, PC_MODE_AUTO, f));                   // a single-pass group never takes the route
    }
    int seen = 0;
    for (const pcn::Group &g : ruled.groups) {
        CHECK(g.two_pass && g.nseg == 1 && g.seg_job.size() == 1 && g.seg_win.size() == 1 && g.seg_adapter.size() == 1);
        CHECK(g.max_window <= 150);                                  // traced windows no longer than the windows themselves
        if (g.nseg != 1 || g.seg_job.size() != 1) continue;
        const int job = g.seg_job[0] >> 1;
        CHECK((g.seg_job[0] & 1) == 0 && g.seg_win[0] == start[job] && g.seg_adapter[0] == adapter[job]);
        CHECK(ruled.seg_first[g.seg_begin] == start[job]);           // (jobs alone: output slots and windows coincide)
        CHECK(pcn::seg_side_of(g, 0, f) == side[job]);
        seen |= 1 << job;
        CHECK(pcn::ruled(p, g, PC_MODE_AUTO, f) && pcn::ruled(p, g, PC_MODE_TWO_PASS, f));
        CHECK(!pcn::ruled(p, g, PC_MODE_TRACE, f) && !pcn::ruled(p, g, PC_MODE_SCORE, f));
        CHECK(!pcn::floored(g, PC_MODE_AUTO, f));                    // (a rule is not a floor)
        pcn::Floors none;
        CHECK(!pcn::ruled(p, g, PC_MODE_AUTO, none));
        pcn::Floors off;
        off.rule_side = no_side;
        CHECK(!pcn::ruled(p, g, PC_MODE_AUTO, off));
        pcn::Params q = p;
        q.end_rule = false;
        CHECK(!pcn::ruled(q, g, PC_MODE_AUTO, f));
    }
    CHECK(seen == 15);
    bool any = false;
    CHECK(pcn::ordered_segments(p, ruled.groups, PC_MODE_AUTO, f, &any) == 4 && any);
    pcn::Floors none;
    CHECK(pcn::ordered_segments(p, ruled.groups, PC_MODE_AUTO, none, &any) == 0 && !any);

    // a dual job: both halves' segments start at the job's first window; the second adapter's records follow the first's
    {
        const int32_t a[1] = {1}, b[1] = {0};
        const int64_t st[2] = {40, 1040};
        const int32_t sd[1] = {0};
        pcn::Table t;
        CHECK(pcn::build_table(panel, p, a, b, st, 1, 150, PC_MODE_AUTO, t) == PC_OK);
        CHECK(t.groups.size() == 1 && t.total == 2000);
        const pcn::Group &g = t.groups[0];
        CHECK(g.two_pass && g.nseg == 2 && g.runs.size() == 1 && g.runs[0].dual);       // not split: one read stream
        CHECK(g.seg_win[0] == 40 && g.seg_win[1] == 40 && g.seg_adapter[0] == 1 && g.seg_adapter[1] == 0);
        CHECK(t.seg_first[g.seg_begin] == 0 && t.seg_first[g.seg_begin + 1] == 1000);
        pcn::Floors fd;
        fd.rule_side = sd;
        CHECK(pcn::ruled(p, g, PC_MODE_AUTO, fd) && pcn::seg_side_of(g, 1, fd) == 0);
    }
    // more segments in one group than the kernels' rule table holds: traced in full
    {
        std::vector<int32_t> a(pck::kRuleSegments + 1, 4), sd(pck::kRuleSegments + 1, 1);
        std::vector<int64_t> st(pck::kRuleSegments + 2);
        for (size_t k = 0; k < st.size(); ++k) st[k] = 100 * (int64_t)k;
        pcn::Table t;
        CHECK(pcn::build_table(panel, p, a.data(), nullptr, st.data(), (int)a.size(), 150, PC_MODE_AUTO, t) == PC_OK);
        CHECK(t.groups.size() == 1 && t.groups[0].nseg == (size_t)pck::kRuleSegments + 1);
        pcn::Floors fm;
        fm.rule_side = sd.data();
        CHECK(!pcn::ruled(p, t.groups[0], PC_MODE_AUTO, fm));
        a.pop_back(); sd.pop_back(); st.pop_back();
        CHECK(pcn::build_table(panel, p, a.data(), nullptr, st.data(), (int)a.size(), 150, PC_MODE_AUTO, t) == PC_OK);
        CHECK(t.groups.size() == 1 && pcn::ruled(p, t.groups[0], PC_MODE_AUTO, fm));
    }
    printf("bad=%d \n", bad);
    return bad ? 1 : 0;
}
