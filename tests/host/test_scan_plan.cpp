// The scan's launch plan (porechop_amd/csrc/pc_scan_plan.h), host-compiled and checked as a plan: seeded job lists plus fixed
// edge cases, over every mode, four scoring schemes (drifting, linear, one whose drift period is below 64 columns, one the
// packed kernels refuse) and both table options.  Per job list:
//   coverage    every run expanded with pck::expand_tile (the function the device's expansion kernel calls) + the plain-int32
//               jobs write every output slot once, with the (window, adapter) the contract above pcn::build_table names
//   structure   tile ranges, ascending tile0, rows, generic groups, the two-pass rule, merge and split under the options
//   segments    one per run half, seg_first, seg_job, the blocks of a segment
//   score pass  the launches of every two-pass group under a fake kernel lookup: partition, merging, heads and tails, regions
//   scratch     alignment and disjointness of the groups' regions
// and, over a grid of shapes, the chunk and grid rules; a hand-made group of 40 M-pair jobs for the tail budget.
//   usage: test_scan_plan [lists [seed]]  ->  bad=0 lists=N merge=... split=... slow=... generic=... tail=... ragged=...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "pc_scan_plan.h"

static long bad = 0, g_list = 0;
static unsigned long long g_seed = 20240611ull;
static void fail(const char *what, long a = 0, long b = 0)
{
    if (++bad <= 25) printf("FAIL %s: seed=%llu list=%ld (%ld, %ld)\n", what, g_seed, g_list, a, b);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(#cond, ##__VA_ARGS__); } while (0)

struct Rng {
    std::mt19937_64 g;
    explicit Rng(unsigned long long s) : g(s) {}
    int below(int n) { return (int)(g() % (unsigned long long)n); }
    bool chance(int percent) { return below(100) < percent; }
    template <typename T> const T &pick(const std::vector<T> &v) { return v[below((int)v.size())]; }
};

struct Scheme { int match, mismatch, open, extend; int longest; };      // longest adapter the panel holds under it
// the panel as pc_api.cpp's upload_panel prepares it
struct TestPanel {
    std::vector<int> len, window;
    std::vector<char> slow;
    pcn::Panel view() const { return pcn::Panel{(int)len.size(), len.data(), window.data(), slow.data()}; }
};
static TestPanel make_panel(const Scheme &s)
{
    TestPanel p;
    std::vector<int> lens = {129, 4096};
    for (int r : pck::kPaddedRows) { lens.push_back(r - 1); lens.push_back(r); lens.push_back(r + 1); }
    for (int r : pck::kExactRows) lens.push_back(r);
    std::sort(lens.begin(), lens.end());
    lens.erase(std::unique(lens.begin(), lens.end()), lens.end());
    int maxm = 1;
    for (int l : lens) if (l <= s.longest || l > pcb::MAX_ADAPTER) { p.len.push_back(l); if (l <= pcb::MAX_ADAPTER) maxm = std::max(maxm, l); }
    const bool slow_scheme = !pcb::scores_supported(s.match, s.mismatch, s.open, s.extend, maxm);
    for (int l : p.len) {
        pcb::Bounds b;
        const bool slow = slow_scheme || l > pcb::MAX_ADAPTER || !pcb::compute_bounds(s.match, s.mismatch, s.open, s.extend, l, b);
        p.slow.push_back(slow ? 1 : 0);
        p.window.push_back(slow ? 0 : b.window);
    }
    return p;
}

struct Jobs { std::vector<int32_t> a, b; std::vector<int64_t> start; };
static void add_job(Jobs &j, int a, int b, int64_t n) { j.a.push_back(a); j.b.push_back(b); j.start.push_back(j.start.back() + n); }
static int own_class(int m_lo, int m_hi, bool no_drift) { bool pad; return no_drift ? std::max(m_lo, m_hi) : pck::pick_rows(m_lo, m_hi, &pad); }

static long n_merge = 0, n_split = 0, n_slow = 0, n_generic = 0, n_tail = 0, n_ragged = 0;

// the fake kernel lookup: by adapter pair none, or a kernel with 1, 2 or 3 workgroups a CU
static int fake_blocks(int lo, int hi) { return (lo * 31 + hi * 7) % 4; }

static void check_score_pass(const pcn::Params &p, const pcn::Group &g, int max_len, int64_t npairs, bool *tail_seen, bool *ragged_seen)
{
    const int gc = pcn::group_chunks_for(p, g, max_len);
    const bool ragged = pcn::ragged_lengths(p, max_len);
    const int plain = pcn::chunks_for((int64_t)g.tile_count, pcn::resident_waves(p, g), max_len, g.max_window);
    CHECK(gc >= 1 && gc <= (ragged ? pcn::kMaxChunksLong : pcn::kMaxChunks), gc);
    if (!ragged) CHECK(gc == plain, gc, plain);
    if (ragged && gc > plain) *ragged_seen = true;
    std::vector<std::pair<int, int>> asked, want;
    auto lookup = [&](int lo, int hi, double cells) {
        CHECK(cells >= 0.0);
        asked.push_back({lo, hi});
        const int bpc = fake_blocks(lo, hi);
        return pcn::SpecKernel{bpc ? (void *)&asked : nullptr, bpc};
    };
    size_t need = 0;
    const std::vector<pcn::ScoreLaunch> L = pcn::plan_score_launches(p, g, max_len, npairs, gc, lookup, &need);
    const bool linear = pcb::is_linear(p.gap_open, p.gap_extend);
    for (size_t i = 0; i < g.runs.size(); ++i)
        if (!linear && (i == 0 || g.runs[i].adapter_lo != g.runs[i - 1].adapter_lo || g.runs[i].adapter_hi != g.runs[i - 1].adapter_hi))
            want.push_back({g.runs[i].adapter_lo, g.runs[i].adapter_hi});
    CHECK(asked == want, (long)asked.size(), (long)want.size());       // once per adapter pair, in table order
    // every tile's slots, to find a launch's pairs
    std::vector<int64_t> tile_lo(g.tile_count), tile_hi(g.tile_count);  // [lowest, highest + 1) output slot of a tile
    for (const pck::TileRun &r : g.runs)
        for (int64_t k = 0; k < pcn::run_tiles(r); ++k) {
            const pck::Tile t = pck::expand_tile(r, k);
            int64_t lo = INT64_MAX, hi = -1;
            if (t.count_lo) { lo = std::min(lo, t.out_lo); hi = std::max(hi, t.out_lo + t.count_lo); }
            if (t.count_hi) { lo = std::min(lo, t.out_hi); hi = std::max(hi, t.out_hi + t.count_hi); }
            tile_lo[r.tile0 + k] = lo; tile_hi[r.tile0 + k] = hi;
        }
    struct Region { int64_t b, e; };
    std::vector<Region> regions = {{0, npairs * 4 * gc}};
    size_t at = 0;
    int64_t k1_run = npairs * 4 * gc;
    for (size_t i = 0; i < L.size(); ++i) {
        const pcn::ScoreLaunch &l = L[i];
        CHECK(l.begin == at && l.count > 0, (long)l.begin, (long)at);
        at = l.begin + l.count;
        const bool tail = i > 0 && l.spec && L[i - 1].spec && L[i - 1].adapter_lo == l.adapter_lo && L[i - 1].adapter_hi == l.adapter_hi;
        if (!l.spec) {
            CHECK(l.chunks == gc && l.k1_ints == 0);
            // pairs without a kernel share a launch whenever they are contiguous with equal chunks: two such launches never touch
            if (i > 0) CHECK(L[i - 1].spec != nullptr);
        }
        if (l.spec) CHECK(l.blocks_per_cu == fake_blocks(l.adapter_lo, l.adapter_hi));
        int64_t lo = INT64_MAX, hi = -1;
        for (size_t t = l.begin; t < l.begin + l.count; ++t) { lo = std::min(lo, tile_lo[t]); hi = std::max(hi, tile_hi[t]); }
        if (!tail) {
            CHECK(l.chunks == gc && l.k1_ints == 0, l.chunks, (long)l.k1_ints);
            CHECK(lo >= 0 && hi <= npairs, (long)lo, (long)hi);                 // [q * 4 * chunks, + 4 * chunks) inside [0, npairs * 4 * chunks)
            continue;
        }
        *tail_seen = true;
        const pcn::ScoreLaunch &h = L[i - 1];
        const size_t slots = (size_t)p.ncu * (size_t)l.blocks_per_cu;
        CHECK(gc == 1 && h.count % slots == 0 && h.count > 0 && l.chunks >= 2 && l.chunks <= 8, (long)h.count, l.chunks);
        CHECK(h.begin + h.count == l.begin);
        CHECK(max_len / l.chunks >= std::max(128, g.max_window / 2));
        // the job's slots: those of head and tail together
        int64_t jlo = lo, jhi = hi;
        for (size_t t = h.begin; t < h.begin + h.count; ++t) { jlo = std::min(jlo, tile_lo[t]); jhi = std::max(jhi, tile_hi[t]); }
        const int64_t rb = l.k1_ints + jlo * 4 * l.chunks, re = rb + (jhi - jlo) * 4 * l.chunks;
        CHECK(rb == k1_run, (long)rb, (long)k1_run);                            // the regions follow one another
        CHECK(l.k1_ints + lo * 4 * l.chunks >= rb && l.k1_ints + hi * 4 * l.chunks <= re);
        // the budget rule held when this tail was granted
        CHECK(((size_t)k1_run + (size_t)(jhi - jlo) * 4 * 8) * 4 <= ((size_t)6 << 30) + (size_t)npairs * 16);
        regions.push_back({rb, re});
        k1_run = re;
    }
    CHECK(at == g.tile_count, (long)at, (long)g.tile_count);
    for (size_t i = 1; i < regions.size(); ++i) CHECK(regions[i].b >= regions[i - 1].e && regions[i].e > regions[i].b);
    CHECK((int64_t)need == regions.back().e, (long)need, (long)regions.back().e);
}

static void check_list(const Scheme &sc, const TestPanel &tp, const Jobs &j, int max_len, int mode, pcn::Params p)
{
    ++g_list;
    p.match = sc.match; p.mismatch = sc.mismatch; p.gap_open = sc.open; p.gap_extend = sc.extend;
    const int njobs = (int)j.a.size();
    const bool no_drift = sc.extend < 0 && pcn::drift_period(sc.open, sc.extend) < 64;       // (only schemes the packed kernels take drift)
    pcn::Table t;
    const int rc = pcn::build_table(tp.view(), p, j.a.data(), j.b.data(), j.start.data(), njobs, max_len, mode, t);
    CHECK(rc == PC_OK, rc);
    if (rc != PC_OK) return;
    auto written_rule = [&](int window) { return mode == PC_MODE_TWO_PASS || mode == PC_MODE_SCORE || mode == PC_MODE_TRACE_AT ||
                                                 (mode == PC_MODE_AUTO && max_len > 2 * window + 64); };
    // ---- the contract ----
    std::vector<int64_t> out_start(njobs + 1, 0);
    for (int k = 0; k < njobs; ++k) out_start[k + 1] = out_start[k] + (j.start[k + 1] - j.start[k]) * (j.b[k] >= 0 ? 2 : 1);
    const int64_t total = out_start[njobs];
    CHECK(t.total == total, (long)t.total, (long)total);
    std::vector<int64_t> want_win(total), got_win(total, -1);
    std::vector<int32_t> want_ad(total), got_ad(total, -1);
    std::map<int64_t, int32_t> seg_owner;                       // first slot of a half with windows -> 2 * job + half
    for (int k = 0; k < njobs; ++k) {
        const int64_t n = j.start[k + 1] - j.start[k];
        for (int half = 0; half < (j.b[k] >= 0 ? 2 : 1); ++half) {
            if (n > 0) seg_owner[out_start[k] + half * n] = 2 * k + half;
            for (int64_t i = 0; i < n; ++i) { want_win[out_start[k] + half * n + i] = j.start[k] + i; want_ad[out_start[k] + half * n + i] = half ? j.b[k] : j.a[k]; }
        }
    }
    auto write = [&](int64_t slot, int64_t win, int32_t ad) {
        if (slot < 0 || slot >= total) { fail("slot outside", (long)slot, (long)total); return; }
        if (got_win[slot] != -1) { fail("slot written twice", (long)slot); return; }
        got_win[slot] = win; got_ad[slot] = ad;
    };
    // ---- structure, and the expansion ----
    size_t next_tile = 0;
    bool merged = false, generic = false;
    for (const pcn::Group &g : t.groups) {
        CHECK(g.tile_begin == next_tile && g.tile_count > 0, (long)g.tile_begin, (long)next_tile);
        next_tile += g.tile_count;
        CHECK((g.rows == 0) == no_drift, g.rows);
        generic |= g.rows == 0;
        int64_t t0 = 0;
        for (const pck::TileRun &r : g.runs) {
            CHECK(r.tile0 == t0 && r.n > 0, (long)r.tile0, (long)t0);
            t0 += pcn::run_tiles(r);
            const int w = std::max(tp.window[r.adapter_lo], tp.window[r.adapter_hi]);
            CHECK(g.two_pass == written_rule(w), mode, w);
            const int own = own_class(tp.len[r.adapter_lo], tp.len[r.adapter_hi], no_drift);
            CHECK(r.rows >= tp.len[r.adapter_lo] && r.rows >= tp.len[r.adapter_hi] && r.rows <= 2 * own && own > 0, r.rows, own);
            if (g.rows) CHECK(r.rows == g.rows, r.rows, g.rows);
            if (p.opt.no_merge_small) CHECK(r.rows == own, r.rows, own);
            merged |= r.rows != own;
            if (mode != PC_MODE_TRACE_AT) CHECK(g.max_window >= w, g.max_window, w);
        }
        CHECK((size_t)t0 == g.tile_count);
        const bool segments = ((!g.two_pass || mode == PC_MODE_TRACE_AT) && g.rows > 0) || (g.two_pass && mode == PC_MODE_TWO_PASS);
        CHECK((g.nseg > 0) == segments && g.seg_job.size() == g.nseg, (long)g.nseg);
        if (!segments) continue;
        size_t s = 0, b = g.blk_begin;
        for (const pck::TileRun &r : g.runs)
            for (int half = 0; half < (r.dual ? 2 : 1); ++half, ++s) {
                if (s >= g.nseg) break;
                const int64_t first = r.out0 + (half ? r.n : 0);
                CHECK(t.seg_first[g.seg_begin + s] == first, (long)s);
                CHECK(seg_owner.count(first) && g.seg_job[s] == seg_owner[first], (long)s, g.seg_job[s]);
                int64_t done = 0;
                while (done < r.n && b < g.blk_begin + g.nblk) {
                    const pck::BucketBlock &bb = t.blocks[b++];
                    CHECK(bb.segment == (int32_t)s && bb.first == first + done && bb.count > 0 && bb.count <= pck::kBucketBlock, (long)s, bb.count);
                    done += bb.count;
                }
                CHECK(done == r.n, (long)done, (long)r.n);
            }
        CHECK(s == g.nseg && b == g.blk_begin + g.nblk, (long)s, (long)g.nseg);
    }
    CHECK(next_tile == t.ntiles, (long)next_tile, (long)t.ntiles);
    int64_t tile0 = 0;
    for (const pck::TileRun &r : t.runs) {
        CHECK(r.tile0 == tile0, (long)r.tile0, (long)tile0);                    // ascending: the device's binary search
        tile0 += pcn::run_tiles(r);
        for (int64_t k = 0; k < pcn::run_tiles(r); ++k) {
            const pck::Tile tl = pck::expand_tile(r, k);
            CHECK(tl.rows >= tp.len[tl.adapter_lo] && tl.rows >= tp.len[tl.adapter_hi]);
            CHECK(tl.count_lo >= 0 && tl.count_lo <= 64 && tl.count_hi >= 0 && tl.count_hi <= 64 && tl.count_lo + tl.count_hi > 0);
            for (int i = 0; i < tl.count_lo; ++i) write(tl.out_lo + i, tl.win_lo + i, tl.adapter_lo);
            for (int i = 0; i < tl.count_hi; ++i) write(tl.out_hi + i, tl.win_hi + i, tl.adapter_hi);
        }
    }
    CHECK((size_t)tile0 == t.ntiles);
    for (const pcn::SlowJob &sj : t.slow_jobs)
        for (int64_t i = 0; i < sj.n; ++i) write(sj.out_base + i, sj.win_start + i, sj.adapter);
    long wrong = 0;
    for (int64_t s = 0; s < total; ++s) wrong += got_win[s] != want_win[s] || got_ad[s] != want_ad[s];
    CHECK(wrong == 0, wrong, (long)total);
    // ---- dual jobs: one run, or two single runs with the same layout ----
    std::map<int64_t, const pck::TileRun *> run_at;
    for (const pck::TileRun &r : t.runs) run_at[r.out0] = &r;
    bool split = false;
    for (int k = 0; k < njobs; ++k) {
        const int64_t n = j.start[k + 1] - j.start[k];
        if (j.b[k] < 0 || n == 0 || tp.slow[j.a[k]] || tp.slow[j.b[k]]) continue;
        const int ma = tp.len[j.a[k]], mb = tp.len[j.b[k]];
        const bool end_window = !written_rule(std::max(tp.window[j.a[k]], tp.window[j.b[k]]));
        const bool differ = own_class(ma, ma, false) != own_class(mb, mb, false);
        const pck::TileRun *r = run_at.count(out_start[k]) ? run_at[out_start[k]] : nullptr;
        CHECK(r != nullptr, k);
        if (!r) continue;
        if (end_window && differ && !no_drift && !p.opt.no_split_dual) {
            const pck::TileRun *r2 = run_at.count(out_start[k] + n) ? run_at[out_start[k] + n] : nullptr;
            CHECK(r2 && !r->dual && !r2->dual && r->n == n && r2->n == n && r->adapter_lo == j.a[k] && r2->adapter_lo == j.b[k], k);
            split = true;
        } else {
            CHECK(r->dual && r->n == n && r->adapter_lo == j.a[k] && r->adapter_hi == j.b[k], k);
        }
    }
    // ---- the scratch layout ----
    const pcn::Scratch sl = pcn::scratch_layout(p, t.groups, max_len, mode);
    struct Span { size_t b, e; };
    std::vector<Span> slab, fin;
    size_t shared_slab = 0, shared_fin = 0;
    for (size_t gi = 0; gi < t.groups.size(); ++gi) {
        const pcn::Group &g = t.groups[gi];
        size_t stride;
        const int grid = pcn::grid_for(p, g, g.tile_count, g.two_pass ? g.max_window + 1 : max_len, &stride);
        CHECK(sl.slab_off[gi] % 256 == 0 && sl.fin_off[gi] % 256 == 0);
        if (!g.two_pass) {
            slab.push_back({sl.slab_off[gi], sl.slab_off[gi] + (size_t)grid * stride * 4});
            fin.push_back({sl.fin_off[gi], sl.fin_off[gi] + (size_t)grid * (size_t)pcn::group_rows(g) * 512});
            continue;
        }
        // behind the single-pass groups' regions, one region for all: large enough for this group's slab and both last-column regions
        shared_slab = sl.slab_off[gi]; shared_fin = sl.fin_off[gi];
        CHECK(sl.slab_off[gi] + (size_t)grid * stride * 4 <= sl.slab_bytes);
        CHECK(sl.fin_region[gi] >= (size_t)grid * (size_t)pcn::group_rows(g) * 512 * 2);
        CHECK(sl.fin_off[gi] + sl.fin_region[gi] * (mode == PC_MODE_SCORE ? 2 : 1) <= sl.fin_bytes);     // the alternate region lies inside
    }
    for (std::vector<Span> *v : {&slab, &fin}) {
        std::sort(v->begin(), v->end(), [](const Span &x, const Span &y) { return x.b < y.b; });
        for (size_t i = 1; i < v->size(); ++i) CHECK((*v)[i].b >= (*v)[i - 1].e, (long)i);
    }
    if (sl.any_two && !slab.empty()) CHECK(shared_slab >= slab.back().e && shared_fin >= fin.back().e);
    if (!slab.empty()) CHECK(slab.back().e <= sl.slab_bytes && fin.back().e <= sl.fin_bytes);
    CHECK(sl.n_single == (int)slab.size());
    // ---- the score pass of the two-pass groups ----
    bool tail = false, ragged = false;
    for (const pcn::Group &g : t.groups)
        if (g.two_pass && mode != PC_MODE_TRACE_AT) check_score_pass(p, g, max_len, total, &tail, &ragged);
    n_merge += merged; n_split += split; n_slow += !t.slow_jobs.empty(); n_generic += generic; n_tail += tail; n_ragged += ragged;
}

// chunks and grids over a grid of shapes
static void check_chunks_and_grids()
{
    for (int64_t tiles : {1, 10, 100, 625, 3000, 6143, 6144, 6145, 50000, 2000000})
    for (int rows : {0, 16, 28, 72, 128})
    for (int max_len : {100, 150, 1000, 8000, 100000, 4000000})
    for (int max_window : {100, 300, 1200})
    for (int ncu : {1, 64, 256})
    for (int len_hint : {0, 2000, 20000}) {
        pcn::Params p;
        p.ncu = ncu; p.len_hint = len_hint;
        pcn::Group g;
        g.rows = rows; g.gen_max_rows = rows ? rows : 40; g.pad = true; g.two_pass = true;
        g.tile_begin = 0; g.tile_count = (size_t)tiles; g.max_window = max_window;
        g.runs.push_back(pck::TileRun{0, 0, tiles * 128, 0, 0, 0, rows ? rows : 40, 0});
        const int cap = pcn::resident_waves(p, g);
        const int plain = pcn::chunks_for(tiles, cap, max_len, max_window), gc = pcn::group_chunks_for(p, g, max_len);
        const bool ragged = pcn::ragged_lengths(p, max_len);
        CHECK(cap >= ncu * 4 && cap <= ncu * 32, cap);
        if (2 * tiles > cap) CHECK(plain == 1, plain);
        CHECK(plain >= 1 && plain <= pcn::kMaxChunks, plain);
        // cut by the under-filled rule: no chunk shorter than the warm-up allows
        if (plain > 1) CHECK((max_len + plain - 1) / plain >= std::max(128, max_window / 2), plain);
        CHECK(gc >= plain && gc <= (ragged ? pcn::kMaxChunksLong : pcn::kMaxChunks) && (ragged || gc == plain), gc, plain);
        // the ragged rule raises the count beyond kMaxChunks only as far as the [pair][chunk] buffer stays below 4 GiB (up to
        // kMaxChunks the buffer is what an unhinted call may take as well)
        if (gc > pcn::kMaxChunks) CHECK(tiles * 128 * 16 * gc <= ((int64_t)4 << 30), gc);
        for (int slab_cols : {1, max_window + 1, max_len})
        for (size_t nt : {(size_t)tiles, (size_t)tiles * (size_t)gc}) {
            size_t stride = 0;
            const int grid = pcn::grid_for(p, g, nt, slab_cols, &stride);
            CHECK(grid >= 1 && (size_t)grid <= nt, grid);
            CHECK(stride == (size_t)slab_cols * (size_t)((g.gen_max_rows + 3) / 4) * 64, (long)stride);
            CHECK(grid == 1 || (size_t)grid * stride * 4 <= ((size_t)8 << 30), grid);     // (one workgroup's slab is what it is)
        }
        for (int force : {1, 4, 64, 1000}) {
            p.opt.force_chunks = force;
            CHECK(pcn::group_chunks_for(p, g, max_len) == std::min(force, std::min(pcn::kMaxChunks, std::max(1, max_len / std::max(128, max_window / 2)))), force);
        }
    }
}

// identical jobs of 40 M pairs each: the chunked tails stop once the tails of the call would leave their budget
static void check_tail_budget()
{
    pcn::Params p;
    p.ncu = 256;
    pcn::Group g;
    g.rows = 36; g.gen_max_rows = 36; g.pad = true; g.two_pass = true; g.tile_begin = 0; g.max_window = 300;
    const int64_t n = 20000000 + 64;               // 312 501 tiles: one over a multiple of every slot count below
    int64_t tile0 = 0, out0 = 0;
    const int njobs = 8;
    for (int k = 0; k < njobs; ++k) { g.runs.push_back(pck::TileRun{0, out0, n, tile0, 2 * k, 2 * k + 1, 36, 1}); tile0 += (n + 63) / 64; out0 += 2 * n; }
    g.tile_count = (size_t)tile0;
    size_t need = 0;
    auto lookup = [](int, int, double) { return pcn::SpecKernel{(void *)&bad, 1}; };
    const std::vector<pcn::ScoreLaunch> L = pcn::plan_score_launches(p, g, 8000, out0, 1, lookup, &need);
    size_t k1 = (size_t)out0 * 4, i = 0;
    bool stopped = false;
    for (int k = 0; k < njobs; ++k) {
        const bool fits = (k1 + (size_t)(2 * n) * 4 * 8) * 4 <= ((size_t)6 << 30) + (size_t)out0 * 16;
        CHECK(i < L.size());
        if (i >= L.size()) return;
        const bool has_tail = i + 1 < L.size() && L[i + 1].adapter_lo == L[i].adapter_lo;
        CHECK(has_tail == fits, k, (long)fits);
        stopped |= !fits;
        if (has_tail) { k1 += (size_t)(2 * n) * 4 * (size_t)L[i + 1].chunks; i += 2; } else i += 1;
    }
    CHECK(stopped && i == L.size() && need == k1, (long)i, (long)L.size());
}

int main(int argc, char **argv)
{
    const long lists = argc > 1 ? atol(argv[1]) : 400;
    if (argc > 2) g_seed = strtoull(argv[2], nullptr, 10);
    Rng rng(g_seed);
    const std::vector<Scheme> schemes = {{3, -6, -5, -2, 128}, {3, -6, -5, -5, 128}, {3, -6, -5, -130, 57}, {3, -6, -5, 0, 128}};
    // (the refused one has no gap extension at all: nothing of the plan may divide by it)
    std::vector<TestPanel> panels;
    for (const Scheme &s : schemes) panels.push_back(make_panel(s));
    CHECK(pcn::drift_period(-5, -2) >= 64 && pcn::drift_period(-5, -5) == 0 && pcn::drift_period(-5, -130) > 0 && pcn::drift_period(-5, -130) < 64);
    CHECK(!panels[2].slow[0] && panels[3].slow[0]);
    const std::vector<int64_t> counts = {0, 1, 63, 64, 65, 127, 128, 129}, big = {2047 * 128, 2048 * 128, 2047 * 128 + 1, 1000 * 64 + 1};
    const std::vector<int> modes = {PC_MODE_AUTO, PC_MODE_TRACE, PC_MODE_TWO_PASS, PC_MODE_SCORE, PC_MODE_TRACE_AT};
    auto index_of = [](const TestPanel &tp, int len) { return (int)(std::find(tp.len.begin(), tp.len.end(), len) - tp.len.begin()); };
    // fixed cases, drifting scheme, end windows: a 16-row class of 2 047 tiles takes the small 20-row class along, one of 2 048 does
    // not; a two-adapter job of two row classes, split and kept dual; and whole reads whose last round is one tile (a chunked tail)
    for (int opt = 0; opt < 4; ++opt)
        for (int64_t n16 : {2047 * 128, 2048 * 128}) {
            const TestPanel &tp = panels[0];
            pcn::Params p;
            p.opt.no_split_dual = opt & 1; p.opt.no_merge_small = (opt & 2) != 0;
            Jobs j; j.start.push_back(0);
            add_job(j, index_of(tp, 16), -1, n16);
            add_job(j, index_of(tp, 20), -1, 129);
            add_job(j, index_of(tp, 24), index_of(tp, 33), 65);
            const long before = n_merge;
            check_list(schemes[0], tp, j, 150, PC_MODE_TRACE, p);
            if (!opt) CHECK((n_merge > before) == true);
        }
    {
        const TestPanel &tp = panels[0];
        pcn::Params p;
        p.ncu = 4;
        Jobs j; j.start.push_back(0);
        for (int k = 0; k < 6; ++k) add_job(j, index_of(tp, 24 + 2 * k), index_of(tp, 28), 1000 * 64 + 1);
        check_list(schemes[0], tp, j, 8000, PC_MODE_TWO_PASS, p);
        p.len_hint = 2000;
        check_list(schemes[0], tp, j, 100000, PC_MODE_TWO_PASS, p);
    }
    while (g_list < lists) {
        const int si = rng.below((int)schemes.size());
        const TestPanel &tp = panels[si];
        pcn::Params p;
        p.ncu = rng.pick(std::vector<int>{1, 4, 64, 256});
        p.len_hint = rng.chance(30) ? rng.pick(std::vector<int>{500, 2000, 20000}) : 0;
        p.opt.no_split_dual = rng.chance(30); p.opt.no_merge_small = rng.chance(30);
        const int mode = rng.pick(modes);
        Jobs j; j.start.push_back(0);
        const int njobs = 1 + rng.below(8);
        int wmax = 1;
        for (int k = 0; k < njobs; ++k) {
            const int a = rng.below((int)tp.len.size());
            int b = -1;
            const int shape = rng.below(3);                 // one adapter; two of one row class; two of different classes
            if (shape) {
                for (int tries = 0; tries < 50; ++tries) {
                    b = rng.below((int)tp.len.size());
                    const bool same = own_class(tp.len[a], tp.len[a], false) == own_class(tp.len[b], tp.len[b], false);
                    if (same == (shape == 1)) break;
                }
            }
            add_job(j, a, b, rng.chance(8) ? rng.pick(big) : rng.pick(counts));
            wmax = std::max(wmax, std::max(tp.window[a], b >= 0 ? tp.window[b] : 0));
        }
        // max_len on both sides of 2 * window + 64 of the list's widest window, the end-window length, and whole reads
        const int max_len = rng.pick(std::vector<int>{150, 2 * wmax + 64, 2 * wmax + 65, 8000, 120000});
        check_list(schemes[si], tp, j, max_len, mode, p);
    }
    // the error returns, in their order
    {
        const TestPanel &tp = panels[0];
        pcn::Params p;
        pcn::Table t;
        const int32_t a_bad[2] = {0, (int32_t)tp.len.size()}, b_none[2] = {-1, -1}, a_ok[2] = {0, 1}, b_bad[2] = {-1, (int32_t)tp.len.size()};
        const int64_t st[3] = {0, 5, 9}, st_neg[3] = {0, 5, 4};
        CHECK(pcn::build_table(tp.view(), p, a_bad, b_none, st, 2, 150, PC_MODE_TRACE, t) == PC_ERR_BAD_ARG);
        CHECK(pcn::build_table(tp.view(), p, a_ok, b_bad, st, 2, 150, PC_MODE_TRACE, t) == PC_ERR_BAD_ARG);
        CHECK(pcn::build_table(tp.view(), p, a_ok, b_none, st_neg, 2, 150, PC_MODE_TRACE, t) == PC_ERR_BAD_ARG);
        CHECK(pcn::build_table(tp.view(), p, a_ok, nullptr, st, 2, 150, PC_MODE_TRACE, t) == PC_OK && t.total == 9);
    }
    check_chunks_and_grids();
    check_tail_budget();
    printf("bad=%ld lists=%ld merge=%ld split=%ld slow=%ld generic=%ld tail=%ld ragged=%ld\n", bad, g_list, n_merge, n_split, n_slow, n_generic,
           n_tail, n_ragged);
    return bad ? 1 : 0;
}
