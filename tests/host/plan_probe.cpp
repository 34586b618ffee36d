// Which kernels does a scan call launch?  The answer of the headers themselves (porechop_amd/csrc/pc_kernels.h, pc_scan_plan.h,
// pc_bounds.h), host-compiled: the row lists, the groups pcn::build_table makes of a job list, every group's
// pcn::trace16_plan, and the two-pass bounds of an adapter length.  tests/rowclassgen.py builds its cases from these answers and
// tests/test_row_class_cases_cpu.py checks that every row class is launched alone.  No switch is set: the Options are the
// defaults of a run without environment, the device has the 256 compute units of the Params' default.
//
//   stdout, first:   exact R...  /  padded R...  /  trace16 R...
//   stdin, by line:  scheme MATCH MISMATCH OPEN EXTEND      (default 3 -6 -5 -2)
//                    int16_only 0|1                         (pc_set_int16_only)
//                    longest M                              (longest adapter of the panel, default 128: decides with the scheme
//                                                            whether the packed kernels take the panel at all)
//                    bounds M          -> bounds M W SPAN WINDOW            (WINDOW 0: compute_bounds refuses)
//                    f16 ROWS COLS     -> f16 ROWS COLS TRACE16 MAX_COLS    (trace16_plan; MAX_COLS 0: f16_plan refuses)
//                    call MODE MAX_LEN NJOBS, then NJOBS lines  M MB N  (MB -1: one adapter; N windows)
//                                      -> call GROUPS SLOW_JOBS TOTAL, then per group
//                                         group ROWS PAD TWO_PASS TILES COLS TRACE16 MAX_COLS
//                                         (ROWS 0: the LDS-state kernel; COLS: the traced launch's columns)
#include <cstdio>
#include <cstring>
#include <vector>

#include "pc_scan_plan.h"

struct ProbePanel {
    std::vector<int> len, window;
    std::vector<char> slow;
    int add(const pcn::Params &p, int m, bool slow_scheme)
    {
        pcb::Bounds b;
        const bool s = slow_scheme || m > pcb::MAX_ADAPTER || !pcb::compute_bounds(p.match, p.mismatch, p.gap_open, p.gap_extend, m > 0 ? m : 1, b);
        len.push_back(m); slow.push_back(s ? 1 : 0); window.push_back(s ? 0 : b.window);
        return (int)len.size() - 1;
    }
};

static int f16_max_cols(const pcn::Params &p, int rows)
{
    if (rows <= 0) return 0;
    const pcb::F16Plan f = pcb::f16_plan(p.match, p.mismatch, p.gap_open, p.gap_extend, rows);
    return f.ok ? f.max_cols : 0;
}

template <size_t N>
static void print_rows(const char *name, const int (&rows)[N])
{
    printf("%s", name);
    for (int r : rows) printf(" %d", r);
    printf("\n");
}

int main()
{
    print_rows("exact", pck::kExactRows);
    print_rows("padded", pck::kPaddedRows);
    print_rows("trace16", pck::kTrace16Rows);
    pcn::Params p;
    int longest = pcb::MAX_ADAPTER;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char word[32] = "";
        if (sscanf(line, "%31s", word) != 1 || word[0] == '#') continue;
        const char *rest = line + (strstr(line, word) - line) + strlen(word);
        if (!strcmp(word, "scheme")) {
            if (sscanf(rest, "%d %d %d %d", &p.match, &p.mismatch, &p.gap_open, &p.gap_extend) != 4) { printf("error scheme\n"); return 2; }
        } else if (!strcmp(word, "int16_only")) {
            int v = 0;
            if (sscanf(rest, "%d", &v) != 1) { printf("error int16_only\n"); return 2; }
            p.int16_only = v != 0;
        } else if (!strcmp(word, "longest")) {
            if (sscanf(rest, "%d", &longest) != 1 || longest < 1) { printf("error longest\n"); return 2; }
        } else if (!strcmp(word, "bounds")) {
            int m = 0;
            if (sscanf(rest, "%d", &m) != 1 || m < 1) { printf("error bounds\n"); return 2; }
            pcb::Bounds b = {0, 0, 0};
            if (!pcb::compute_bounds(p.match, p.mismatch, p.gap_open, p.gap_extend, m, b)) b = pcb::Bounds{0, 0, 0};
            printf("bounds %d %d %d %d\n", m, b.W, b.SPAN, b.window);
        } else if (!strcmp(word, "f16")) {
            int rows = 0, cols = 0;
            if (sscanf(rest, "%d %d", &rows, &cols) != 2) { printf("error f16\n"); return 2; }
            printf("f16 %d %d %d %d\n", rows, cols, pcn::trace16_plan(p, rows, cols) ? 1 : 0, f16_max_cols(p, rows));
        } else if (!strcmp(word, "call")) {
            int mode = 0, max_len = 0, njobs = 0;
            if (sscanf(rest, "%d %d %d", &mode, &max_len, &njobs) != 3 || njobs < 0 || njobs > 100000) { printf("error call\n"); return 2; }
            const int cap = longest < pcb::MAX_ADAPTER ? longest : pcb::MAX_ADAPTER;
            const bool slow_scheme = !pcb::scores_supported(p.match, p.mismatch, p.gap_open, p.gap_extend, cap);
            ProbePanel panel;
            std::vector<int32_t> ja, jb;
            std::vector<int64_t> start(1, 0);
            for (int k = 0; k < njobs; ++k) {
                int m = 0, mb = -1;
                long long n = 0;
                if (!fgets(line, sizeof line, stdin) || sscanf(line, "%d %d %lld", &m, &mb, &n) != 3 || m < 1 || n < 0) { printf("error job %d\n", k); return 2; }
                ja.push_back(panel.add(p, m, slow_scheme));
                jb.push_back(mb > 0 ? panel.add(p, mb, slow_scheme) : -1);
                start.push_back(start.back() + n);
            }
            const pcn::Panel view{(int)panel.len.size(), panel.len.data(), panel.window.data(), panel.slow.data()};
            pcn::Table t;
            const int rc = pcn::build_table(view, p, ja.data(), jb.data(), start.data(), njobs, max_len, mode, t);
            if (rc) { printf("error build_table %d\n", rc); return 2; }
            printf("call %zu %zu %lld\n", t.groups.size(), t.slow_jobs.size(), (long long)t.total);
            for (const pcn::Group &g : t.groups) {
                const int cols = g.two_pass ? g.max_window + 1 : max_len;
                printf("group %d %d %d %zu %d %d %d\n", g.rows, g.pad ? 1 : 0, g.two_pass ? 1 : 0, g.tile_count, cols,
                       pcn::trace16_plan(p, g.rows, cols) ? 1 : 0, f16_max_cols(p, g.rows));
            }
        } else {
            printf("error unknown %s\n", word);
            return 2;
        }
    }
    return 0;
}
