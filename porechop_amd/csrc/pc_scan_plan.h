// pc_scan_plan.h -- the launch plan of the alignment scan (pc_scan_device and everything built on it), made on the host.
//
// Everything a scan decides before it enqueues anything is decided here: how a job list becomes row-class groups of tile
// runs, segments, bucket blocks, plain-int32 jobs and an output layout; how many column chunks and workgroups a launch
// gets; where every group's scratch lies; how a two-pass group's score pass is cut into launches; which groups run their
// second pass ordered or floored.  No device runtime, no environment, no context: pc_api.cpp reads the switches into
// Options, calls these functions and launches over what they return; tests/host/test_scan_plan.cpp checks the plans
// themselves on the CPU, expanding the runs with the function the device runs (pck::expand_tile).
#pragma once
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "../../include/porechop_amd.h"
#include "pc_bounds.h"
#include "pc_kernels.h"

namespace pcn {

// The environment switches of the scan, as pc_api.cpp read them (there, in one place).
struct Options {
    bool no_split_dual = false;         // PC_NO_SPLIT_DUAL: a two-adapter end-window job stays one dual run
    bool no_merge_small = false;        // PC_NO_MERGE_SMALL: every row class its own launch, however small
    bool f16_disabled = false;          // PC_DISABLE_F16: the traced scan in packed int16 throughout
    bool no_trace_fork = false;         // PC_NO_TRACE_FORK: the single-pass groups on one stream
    bool no_end_order = false;          // PC_NO_END_ORDER: PC_MODE_TRACE_AT takes the pairs as handed over
    bool no_pair_trace_bound = false;   // PC_NO_PAIR_TRACE_BOUND: pass 2 traces the adapter-wide W + 2 columns
    bool no_score_fork = false;         // PC_NO_SCORE_FORK (per call): a score-only call's launches on one stream
    int force_chunks = 0;               // PC_FORCE_CHUNKS (per call); < 1: by the fill
    bool no_end_floor = false;          // PC_NO_END_FLOOR (per call): an end rule handed to the scan is ignored
    bool no_row_skip = false;           // PC_NO_ROW_SKIP (per call): the score pass of a floored call computes every row in every column
};

// What the rules below need to know of the context.
struct Params {
    int ncu = 256;                      // compute units of the device
    int len_hint = 0;                   // pc_set_length_hint
    bool int16_only = false;            // pc_set_int16_only
    int match = 3, mismatch = -6, gap_open = -5, gap_extend = -2;
    bool end_rule = false;              // the call carries an end rule (pc_scan_device_end_rule, and the switch above is off)
    Options opt;
};

// The adapter table: per adapter its length, its pass-2 window (pcb::Bounds::window) and whether it takes the plain-int32 kernel.
struct Panel { int n; const int *len, *window; const char *slow; };

struct Group {            // tiles that run in one launch
    int rows;             // 0: generic kernel
    int gen_max_rows;     // generic: largest adapter in the group
    bool pad;
    bool two_pass;
    size_t tile_begin, tile_count;
    int max_window;       // for two-pass groups: slab columns needed by the traced window
    std::vector<pck::TileRun> runs;   // the group's tiles, run by run (tile0 relative to tile_begin)
    // single-pass groups (end windows): the segments -- runs of output slots with one adapter -- and their pieces, for the
    // two-pass end scan's ordering by end column (pck::launch_bucket_pairs); offsets into the slot's bucket table
    size_t seg_begin = 0, nseg = 0, blk_begin = 0, nblk = 0;
    // two-pass groups of a PC_MODE_TWO_PASS call have them too: the second pass of a floored call puts the pairs below their
    // job's score floor behind the others of their segment.  seg_job[s] = 2 * job + (0: its first adapter, 1: its second)
    std::vector<int32_t> seg_job;
    // ... and so have the two-pass groups of a call with an end rule, which also asks for every segment's first window and
    // adapter (the rule looks at the window's length and names the adapter's)
    std::vector<int64_t> seg_win;
    std::vector<int32_t> seg_adapter;
};

inline int group_rows(const Group &g) { return g.rows ? g.rows : g.gen_max_rows; }
inline int64_t run_tiles(const pck::TileRun &r) { return r.dual ? (r.n + 63) / 64 : (r.n + 127) / 128; }
// pairs in tiles [b, e) of a run
inline int64_t run_pairs(const pck::TileRun &r, int64_t b, int64_t e)
{
    const int64_t w = r.dual ? 64 : 128;
    const int64_t windows = std::min<int64_t>(r.n, w * e) - w * b;
    return windows <= 0 ? 0 : (r.dual ? 2 * windows : windows);
}
// pairs in tiles [b, e) of a group
inline int64_t group_pairs(const Group &g, size_t b, size_t e)
{
    int64_t np = 0;
    for (const pck::TileRun &r : g.runs) {
        const int64_t t0 = r.tile0, t1 = r.tile0 + run_tiles(r);
        const int64_t lo = std::max<int64_t>(t0, (int64_t)b), hi = std::min<int64_t>(t1, (int64_t)e);
        if (lo < hi) np += run_pairs(r, lo - t0, hi - t0);
    }
    return np;
}
inline int64_t group_pairs(const Group &g) { return group_pairs(g, 0, g.tile_count); }

// Columns the register variants' drifting coordinates (the kernels' column_step) can run before
// int16 needs a renormalisation: values drift up by eps = -gap_extend per column on top of a true
// range of at most +-8000 (pcb::scores_supported) and (rows + 2) * eps of row offsets.  0 = the
// scheme cannot drift (linear-gap mode replaces gap_extend by a huge value).
inline int drift_period(int gap_open, int gap_extend)
{
    if (pcb::is_linear(gap_open, gap_extend)) return 0;
    const long eps = -(long)gap_extend;
    const long k = (24000 - (long)(pcb::MAX_ADAPTER + 2) * eps) / eps;
    return (int)std::max<long>(0, std::min<long>(k, 1 << 20));
}

// ---- the table plan ------------------------------------------------------------------------------------------------

// jobs the packed 16-bit kernels cannot take (scheme outside pcb::scores_supported, adapter above pcb::MAX_ADAPTER):
// they run the plain-int32 kernel (pck::launch_slow) after the tiles, each with its place in the output kept
struct SlowJob { int64_t win_start, n, out_base; int adapter; };

struct Table {
    std::vector<Group> groups;                  // the launches, in table order; none is empty
    std::vector<pck::TileRun> runs;             // every group's runs with tile0 over ALL groups: what the device expands
    std::vector<int64_t> seg_first;             // first output slot of every segment
    std::vector<pck::BucketBlock> blocks;       // the segments in pieces of at most pck::kBucketBlock slots
    std::vector<SlowJob> slow_jobs;
    size_t ntiles = 0;
    int64_t total = 0;                          // output slots (pairs) of the call
};

// A pair whose windows of up to max_len columns are scanned score-only first and traced over `window` columns around the best cell
// (end_rule: the call carries an end rule -- then, and only then, PC_MODE_AUTO takes short windows in two passes as well: what
// the first pass costs is won back by the pairs the rule keeps out of the second)
inline bool two_pass_rule(int mode, int max_len, int window, bool end_rule = false)
{
    return mode == PC_MODE_TWO_PASS || mode == PC_MODE_SCORE || mode == PC_MODE_TRACE_AT ||
           (mode == PC_MODE_AUTO && (end_rule || max_len > 2 * window + 64));
}

// The table of a job list.  Job k scans windows [job_start[k], job_start[k+1]) against adapter job_adapter[k] and, when
// job_adapter_b (may be null) has job_adapter_b[k] >= 0, ALSO against that second adapter in the same pass (both halves of
// a lane then read the same window: one read stream instead of two).
// Outputs: out_start(k) = sum over k' < k of n_k' * (1 or 2); adapter A's records first, then B's.
// Returns PC_OK, or PC_ERR_BAD_ARG (then `out` is unspecified).
inline int build_table(const Panel &ad, const Params &p, const int32_t *job_adapter, const int32_t *job_adapter_b,
                       const int64_t *job_start, int njobs, int max_len, int mode, Table &out)
{
    out = Table();
    std::map<std::pair<int, int>, std::vector<pck::TileRun>> by_group;   // (rows*2+pad, two_pass) -> runs
    std::map<std::pair<int, int>, int> group_window;
    std::map<int64_t, int32_t> job_of_first;
    int64_t out_pos = 0;
    for (int k = 0; k < njobs; ++k) {
        const int a = job_adapter[k], adb = job_adapter_b ? job_adapter_b[k] : -1;
        if (a < 0 || a >= ad.n || adb >= ad.n) return PC_ERR_BAD_ARG;
        const int m = ad.len[a], mb = adb >= 0 ? ad.len[adb] : m;
        if (m <= 0 || mb <= 0) return PC_ERR_BAD_ARG;
        const int64_t ws = job_start[k], n = job_start[k + 1] - job_start[k];
        if (n < 0) return PC_ERR_BAD_ARG;
        if (ad.slow[a] || (adb >= 0 && ad.slow[adb])) {
            // no tiles: the plain-int32 kernel runs this job after them (adapter A's records first, then B's)
            if (n > 0) out.slow_jobs.push_back({ws, n, out_pos, a});
            out_pos += n;
            if (adb >= 0) { if (n > 0) out.slow_jobs.push_back({ws, n, out_pos, adb}); out_pos += n; }
            continue;
        }
        // the register variants run in drifting coordinates: linear-gap schemes (extension made
        // impossible, pc_bounds.h) and schemes whose gap extension is too large to drift in int16 take
        // the generic kernel.  (Asked only here: a scheme the packed kernels refuse may have no extension to divide by.)
        const bool no_drift = drift_period(p.gap_open, p.gap_extend) < 64;
        auto group_of = [&](int ma, int mbb, int window, int *rows_out) -> std::vector<pck::TileRun> & {
            bool pad = false;
            int rows = pck::pick_rows(ma, mbb, &pad);         // 0 => generic LDS-state kernel
            if (no_drift) { rows = 0; pad = true; }
            const bool two = two_pass_rule(mode, max_len, window, p.end_rule);
            // PC_MODE_TRACE_AT over short windows: a traced window never needs to be longer than the windows themselves
            // (one that holds its read's column 0 starts from the true column 0: no warm-up before it); a call with an end
            // rule caps its traced windows in the same way (plan_kernel: window_cap)
            if (mode == PC_MODE_TRACE_AT || p.end_rule) window = std::min(window, std::max(1, max_len));
            auto key = std::make_pair(rows * 2 + (pad ? 1 : 0), two ? 1 : 0);
            group_window[key] = std::max(group_window[key], window);
            *rows_out = rows;
            return by_group[key];
        };
        // one adapter, two windows per lane (the halves read different streams): tiles of 128 windows
        auto emit_single = [&](int a1, int64_t out_base) {
            const int m1 = ad.len[a1];
            int rows;
            auto &v = group_of(m1, m1, ad.window[a1], &rows);
            if (n > 0) v.push_back(pck::TileRun{ws, out_base, n, 0, a1, a1, rows ? rows : m1, 0});
        };
        const int window = std::max(ad.window[a], adb >= 0 ? ad.window[adb] : 0);
        // A dual tile runs both halves with the longer adapter's rows and saves the second read stream and
        // the second byte -> row lookup per column.  For whole reads that is worth more than the padding
        // rows -- measured on the headline's four middle adapters, 1 M x 8 kb reads: (33 | 30) + (28 | 22)
        // dual 74.6 ms of pc_spec_score per step, the four adapters alone with two streams per lane 81.3 ms,
        // where dropping the 9 padded rows of 122 could have saved 5.5 ms (profiles/score_layout_ab.txt) --
        // so two-pass jobs stay dual.  For 150-byte end windows two adapters of different row classes cost
        // fewer rows as two single-adapter jobs (same tile count, same output layout).
        bool pa_ = false, pb_ = false;
        const bool split_dual = adb >= 0 && !two_pass_rule(mode, max_len, window, p.end_rule) && !no_drift && !p.opt.no_split_dual &&
                                pck::pick_rows(m, m, &pa_) != pck::pick_rows(mb, mb, &pb_);
        job_of_first[out_pos] = 2 * k;                         // (first record of a segment -> whose it is)
        if (adb >= 0) job_of_first[out_pos + n] = 2 * k + 1;
        if (adb >= 0 && !split_dual) {
            // both halves of a lane scan the same 64 windows: adapter A's records first, then B's
            int rows;
            auto &v = group_of(m, mb, window, &rows);
            if (n > 0) v.push_back(pck::TileRun{ws, out_pos, n, 0, a, adb, rows ? rows : std::max(m, mb), 1});
            out_pos += 2 * n;
        } else if (adb >= 0) {
            emit_single(a, out_pos);
            emit_single(adb, out_pos + n);
            out_pos += 2 * n;
        } else {
            emit_single(a, out_pos);
            out_pos += n;
        }
    }
    out.total = out_pos;
    // Small single-pass groups run together.  A group is one launch; a handful of jobs of a rare adapter length (phase A:
    // 217 of the panel's sequences are 24-mers, the other 19 fall into nine row classes of 80-470 tiles each) ends in a
    // launch that fills a tenth of the chip for the duration of a whole tile, and ten of those in a row cost more than the
    // 24-mers' launch.  Ascending by rows, groups below kSmallTiles are merged into the next larger small group (its rows,
    // padded variant: a shorter adapter sits bottom-aligned under padding rows, as in any tile of two different adapters)
    // until the merged group is large enough; the extra rows are cheap next to an idle chip.  Results do not depend on the
    // row class a pair runs in (tests/test_gpu_row_classes.py: every class launched alone, against the oracle).
    if (!p.opt.no_merge_small) {
        const int64_t kSmallTiles = 2048;
        std::vector<std::pair<int, int>> keys;
        for (auto &kv : by_group) if (kv.first.second == 0 && kv.first.first / 2 > 0) keys.push_back(kv.first);
        std::sort(keys.begin(), keys.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) {
            return x.first / 2 != y.first / 2 ? x.first / 2 < y.first / 2 : x.first < y.first; });
        auto tiles_of = [&](const std::pair<int, int> &k) { int64_t t = 0; for (auto &r : by_group[k]) t += run_tiles(r); return t; };
        auto padded_class = [](int rows) { for (int r : pck::kPaddedRows) if (r == rows) return true; return false; };
        bool have_open = false;
        std::pair<int, int> open;
        int64_t open_tiles = 0;
        int open_min_rows = 0;                                         // (never more than twice the rows a pair needs)
        for (const auto &key : keys) {
            const int64_t t = tiles_of(key);
            if (t >= kSmallTiles) continue;                            // large groups stay as they are
            const int rows_t = key.first / 2;
            if (have_open && key == open) continue;                    // (already the group the smaller classes were merged into)
            if (!have_open || rows_t > 2 * open_min_rows) { have_open = true; open = key; open_tiles = t; open_min_rows = rows_t; continue; }
            if (!padded_class(rows_t) || rows_t < open.first / 2) continue;   // no padded variant of this class: it stays alone
            const std::pair<int, int> target(rows_t * 2 + 1, 0);
            std::vector<pck::TileRun> moved;
            int window = 0;
            const std::pair<int, int> olds[2] = {open, key};
            for (const auto &old : olds) {
                auto it = by_group.find(old);
                if (it == by_group.end()) continue;
                for (auto &r : it->second) { r.rows = rows_t; moved.push_back(r); }
                window = std::max(window, group_window[old]);
                by_group.erase(it);
                group_window.erase(old);
            }
            // (the padded group of this class may exist already -- e.g. 27-mers beside exact 28-mers: joined, not replaced)
            auto &dst = by_group[target];
            for (auto &r : dst) r.rows = rows_t;
            dst.insert(dst.end(), moved.begin(), moved.end());
            group_window[target] = std::max(group_window[target], window);
            open = target; open_tiles += t;
            if (open_tiles >= kSmallTiles) have_open = false;
        }
    }
    for (auto &kv : by_group) {
        Group g;
        g.rows = kv.first.first / 2; g.pad = (kv.first.first & 1) != 0; g.two_pass = kv.first.second != 0;
        g.tile_begin = out.ntiles;
        g.max_window = group_window[kv.first];
        g.gen_max_rows = 1;
        int64_t t = 0;
        for (pck::TileRun &r : kv.second) {
            g.gen_max_rows = std::max(g.gen_max_rows, (int)r.rows);
            r.tile0 = t;
            t += run_tiles(r);
            out.runs.push_back(r);
            out.runs.back().tile0 += (int64_t)g.tile_begin;     // the device table is indexed over all groups
        }
        g.tile_count = (size_t)t;
        g.runs.swap(kv.second);
        out.ntiles += g.tile_count;
        if (((!g.two_pass || mode == PC_MODE_TRACE_AT) && g.rows > 0) || (g.two_pass && (mode == PC_MODE_TWO_PASS || p.end_rule))) {
            g.seg_begin = out.seg_first.size(); g.blk_begin = out.blocks.size();
            for (const pck::TileRun &r : g.runs) {
                for (int half = 0; half < (r.dual ? 2 : 1); ++half) {
                    const int64_t first = r.out0 + (half ? r.n : 0);
                    const int32_t sgm = (int32_t)(out.seg_first.size() - g.seg_begin);
                    out.seg_first.push_back(first);
                    g.seg_job.push_back(job_of_first.at(first));
                    g.seg_win.push_back(r.win0);
                    g.seg_adapter.push_back(half ? r.adapter_hi : r.adapter_lo);
                    for (int64_t at = 0; at < r.n; at += pck::kBucketBlock)
                        out.blocks.push_back(pck::BucketBlock{first + at, (int32_t)std::min<int64_t>(pck::kBucketBlock, r.n - at), sgm});
                }
            }
            g.nseg = out.seg_first.size() - g.seg_begin; g.nblk = out.blocks.size() - g.blk_begin;
        }
        if (g.tile_count) out.groups.push_back(std::move(g));
    }
    if (out.ntiles > (size_t)INT32_MAX) return PC_ERR_BAD_ARG;
    return PC_OK;
}

// ---- chunks and grids ----------------------------------------------------------------------------------------------

constexpr int kMaxChunks = 64, kMaxChunksLong = 2048;

// Column chunks of the score pass.  With enough tiles to fill the chip: 1 (no warm-up overhead).
// Under-filled (small batches, mask-and-realign rounds): the launch's duration is the serial column
// loop of one wave, so cut the windows into as many chunks as there are idle wave slots, down to
// chunks about as long as their SPAN warm-up (exact, see pc_bounds.h).
inline int chunks_for(int64_t tile_count, int capacity, int max_len, int max_window)
{
    if (tile_count <= 0 || tile_count * 2 > capacity) return 1;
    int chunks = (int)std::min<int64_t>(kMaxChunks, capacity / tile_count);
    const int min_len = std::max(128, max_window / 2);
    return std::max(1, std::min(chunks, max_len / min_len));
}

// Resident waves the chip holds for this group's kernels: by register footprint (2 packed VGPRs per
// row + ~48) for the register variants, by LDS (8 B per row per lane) for the generic one.
inline int resident_waves(const Params &p, const Group &g)
{
    const int rows = group_rows(g);
    int per_simd = g.rows ? 512 / (2 * rows + 48) : (int)((160 * 1024) / ((size_t)rows * 520 + 1024)) / 4;
    per_simd = std::max(1, std::min(8, per_simd));
    return p.ncu * 4 * per_simd;
}

// Column chunks of a two-pass group's score pass: the under-filled rule above, or -- reads of very
// different lengths (the caller's typical length is far below the longest, pc_set_length_hint) -- chunks
// about as long as a typical read, so that no unit of work is much longer than the others: a launch
// otherwise lasts as long as its longest read (measured on log-normal lengths, mean 8 kb, longest
// 113 kb: 3.4 times the balanced duration).  The windows come longest first, units are drawn in
// that order (work_counter), and chunks beyond a window's end cost a few microseconds.
inline bool ragged_lengths(const Params &p, int max_len) { return p.len_hint > 0 && (int64_t)max_len * 2 > (int64_t)p.len_hint * 3; }

inline int group_chunks_for(const Params &p, const Group &g, int max_len)
{
    // PC_FORCE_CHUNKS=n (tests): that many column chunks whatever the fill -- 1 runs a whole window in one unit, which a
    // launch otherwise only does when thousands of tiles fill the chip (tests/test_gpu_ultralong.py: columns beyond 65 535
    // through the un-chunked branch of the specialised score kernel without a 20 GB batch)
    if (p.opt.force_chunks >= 1)
        return std::min(p.opt.force_chunks, std::min(kMaxChunks, std::max(1, max_len / std::max(128, g.max_window / 2))));
    int chunks = chunks_for((int64_t)g.tile_count, resident_waves(p, g), max_len, g.max_window);
    if (ragged_lengths(p, max_len)) {
        const int unit = std::max(p.len_hint, std::max(512, 4 * g.max_window));
        // (a batch whose longest read is a hundred times the typical one -- a 4 Mb read among 20 kb reads -- needs more than
        // kMaxChunks units of typical length: up to kMaxChunksLong, as far as the [pair][chunk] pass-1 buffer stays below 4 GiB)
        const int64_t pairs = std::max<int64_t>(1, group_pairs(g));
        const int by_memory = (int)std::max<int64_t>(kMaxChunks, std::min<int64_t>(kMaxChunksLong, ((int64_t)4 << 30) / (pairs * 16)));
        // ... and few windows (a batch of 40 000 long reads is 625 tiles: units of typical length would be a fifth of the wave slots,
        // and the launch would last as long as ONE such unit, 5 ms at 20 kb): then the units are made short enough that there are
        // about three per slot -- the windows' columns, estimated as tiles x typical length, over 3 x the resident waves -- but
        // not shorter than a few warm-up spans
        int unit_len = unit;
        const int64_t slots = resident_waves(p, g);
        const int64_t est_units = (int64_t)g.tile_count * std::max(1, p.len_hint / std::max(1, unit)) ;
        if (est_units < 3 * slots) {
            const int64_t cols = (int64_t)g.tile_count * p.len_hint;
            unit_len = (int)std::max<int64_t>(std::max(512, 4 * g.max_window), std::min<int64_t>(unit, cols / (3 * slots)));
        }
        chunks = std::max(chunks, std::min(by_memory, (max_len + unit_len - 1) / unit_len));
    }
    return chunks;
}

// Workgroups to launch for `ntiles` tiles.  Measured on MI355X (tools/time_score.py, time_trace.py):
// handing the hardware dispatcher one tile per workgroup beats a persistent grid of exactly the
// resident waves striding over the tiles -- 4-5 % on the uniform whole-read score pass, 13 % on the
// traced end windows, whose tiles differ in cost (window lengths, traceback lengths).  The grid is
// therefore the tile count, bounded only by the per-workgroup scratch (trace slab, last-column
// save); above the bound the kernels stride.
constexpr int64_t kMaxGrid = 32768;
inline int grid_for(const Params &p, const Group &g, size_t ntiles, int slab_cols, size_t *slab_stride_dwords)
{
    int64_t grid = std::max<int64_t>(kMaxGrid, resident_waves(p, g));
    const size_t stride = (size_t)std::max(1, slab_cols) * pck::trace_words_per_col(group_rows(g)) * 64;
    const size_t budget = (size_t)8 << 30;    // keep the trace scratch under 8 GiB
    while (grid > 1 && (size_t)grid * stride * 4 > budget) grid = grid * 3 / 4;
    grid = std::min<int64_t>(grid, (int64_t)ntiles);
    if (slab_stride_dwords) *slab_stride_dwords = stride;
    return (int)std::max<int64_t>(1, grid);
}

// The traced scan runs in packed fp16 (trace16_kernel, 13.25 instead of 21 packed ops per
// two cells) whenever the scheme's values stay exact there for the columns of this launch
// (pc_bounds.h f16_plan); otherwise -- linear-gap schemes, very large scores, adapters above 72 rows,
// the LDS-state generic kernel -- in packed int16.  PC_DISABLE_F16=1 forces the int16 kernels.
inline bool trace16_plan(const Params &p, int rows, int cols, pcb::F16Plan *out)
{
    if (p.opt.f16_disabled || p.int16_only || rows <= 0 || !pck::trace16_has(rows)) return false;
    const pcb::F16Plan f = pcb::f16_plan(p.match, p.mismatch, p.gap_open, p.gap_extend, rows);
    if (!f.ok || cols > f.max_cols) return false;
    *out = f;
    return true;
}
inline bool trace16_plan(const Params &p, int rows, int cols) { pcb::F16Plan f; return trace16_plan(p, rows, cols, &f); }

// Pairs per launch of a kernel that needs per_pair bytes of scratch for each of them: what the budget holds, in whole
// waves, and never fewer than one wave, whatever that makes the scratch ...
inline int64_t budget_pairs(size_t budget, size_t per_pair) { return std::max<int64_t>(64, (int64_t)(budget / per_pair) / 64 * 64); }
// ... and no more than the n pairs there are, rounded up to waves
inline int64_t slice_pairs(size_t budget, size_t per_pair, int64_t n) { return std::min<int64_t>(budget_pairs(budget, per_pair), (n + 63) / 64 * 64); }

// ---- the scratch layout --------------------------------------------------------------------------------------------

// Byte offsets of every group's trace slab and last-column save.  Single-pass groups get regions of their own (they run
// concurrently); two-pass groups run one after the other and share the region behind them, sized for the largest.
struct Scratch {
    std::vector<size_t> slab_off, fin_off;      // per group
    std::vector<size_t> fin_region;             // two-pass groups: bytes of one last-column region (a score-only call has two)
    size_t slab_bytes = 0, fin_bytes = 0;       // in all
    int n_single = 0;
    bool any_two = false;
};

inline Scratch scratch_layout(const Params &p, const std::vector<Group> &groups, int max_len, int mode)
{
    Scratch s;
    s.slab_off.assign(groups.size(), 0); s.fin_off.assign(groups.size(), 0); s.fin_region.assign(groups.size(), 0);
    size_t slab_single = 0, fin_single = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group &g = groups[gi];
        size_t stride;
        const int grid = grid_for(p, g, g.tile_count, g.two_pass ? g.max_window + 1 : max_len, &stride);
        const size_t rows = (size_t)std::max(1, group_rows(g));
        if (!g.two_pass) {
            s.slab_off[gi] = slab_single; s.fin_off[gi] = fin_single;
            slab_single += ((size_t)grid * stride * 4 + 255) & ~(size_t)255;
            fin_single += ((size_t)grid * rows * 64 * 8 + 255) & ~(size_t)255;
            ++s.n_single;
            continue;
        }
        s.slab_bytes = std::max(s.slab_bytes, (size_t)grid * stride * 4);
        // score pass: chunked launches, and the chunked tails of big jobs (at most 8 chunks x resident waves)
        const int grid1 = grid_for(p, g, std::max<size_t>(g.tile_count * (size_t)group_chunks_for(p, g, max_len), (size_t)p.ncu * 64), 1, nullptr);
        // (x2: the specialised score kernel parks the two halves of a lane separately)
        // (x2 again for a score-only call: its launches alternate between two streams, each with a region of its own)
        s.fin_region[gi] = (size_t)std::max(grid, grid1) * rows * 64 * 8 * 2;
        s.fin_bytes = std::max(s.fin_bytes, s.fin_region[gi] * (mode == PC_MODE_SCORE ? 2 : 1));
        s.any_two = true;
    }
    for (size_t gi = 0; gi < groups.size(); ++gi)
        if (groups[gi].two_pass) { s.slab_off[gi] = slab_single; s.fin_off[gi] = fin_single; }
    s.slab_bytes += slab_single; s.fin_bytes += fin_single;
    return s;
}

// ---- the score pass of a two-pass group ----------------------------------------------------------------------------

// One launch of the score pass: a run of tiles, each cut into `chunks` column chunks, writing its
// [pair][chunk] maxima at k1_ints of the pass-1 buffer; spec = the run-time specialised kernel of
// the run's adapter pair (the lookup's handle, with the workgroups a CU holds of it), or null for the generic kernel
// (which takes the adapter from each tile).
// k1_ints may be "virtual": the kernels index a launch's region by GLOBAL pair index, a chunked tail's region only
// holds its own job's pairs, so its base is moved back by the job's first pair (never dereferenced below the region).
struct ScoreLaunch { size_t begin, count; int chunks; int64_t k1_ints; void *spec; int blocks_per_cu; int adapter_lo, adapter_hi; };

struct SpecKernel { void *spec; int blocks_per_cu; };       // what the lookup answers; spec == null: none

// Launch plan of a two-pass group.  Tiles of one job (= one adapter pair) are contiguous.  A job
// with a specialised kernel and more tiles than resident waves is launched as a balanced head (a
// multiple of the resident waves, whole windows) plus a tail whose tiles are cut into column
// chunks: the last, partly filled round of whole tiles would idle part of the chip for a whole tile
// (measured 5 % at 7.6 tiles per wave, 11 % at 4.05), the chunked tail fills it.  Each chunked tail
// gets its own region of the pass-1 buffer (its [pair][chunk] indexing differs from the head's).
// lookup(adapter_lo, adapter_hi, estimated cells) -> SpecKernel is asked once per adapter pair, in table order (the
// library's adds the cells to the pair's running total to decide when a kernel is worth its compile), and not at all
// under a linear-gap scheme.
template <typename Lookup>
inline std::vector<ScoreLaunch> plan_score_launches(const Params &p, const Group &g, int max_len, int64_t npairs, int group_chunks,
                                                    Lookup lookup, size_t *k1_ints_needed)
{
    std::vector<ScoreLaunch> out;
    const bool linear = pcb::is_linear(p.gap_open, p.gap_extend);
    size_t k1 = (size_t)npairs * 4 * (size_t)group_chunks;
    size_t ri = 0;
    while (ri < g.runs.size()) {
        // consecutive runs of one adapter pair share their launches
        const pck::TileRun &r0 = g.runs[ri];
        size_t re = ri + 1;
        while (re < g.runs.size() && g.runs[re].adapter_lo == r0.adapter_lo && g.runs[re].adapter_hi == r0.adapter_hi) ++re;
        const size_t i = (size_t)r0.tile0;
        const size_t e = (size_t)(g.runs[re - 1].tile0 + run_tiles(g.runs[re - 1]));
        // the specialised kernel for this pair, once the work seen for the pair has paid for its
        // compile (pc_jit.cpp); until then the generic one
        // (windows of very different lengths: their typical length, not the longest, is what the launch costs)
        const double est_len = ragged_lengths(p, max_len) ? (double)p.len_hint : (double)max_len;
        const double est_cells = (double)group_pairs(g, i, e) * est_len * (double)group_rows(g);
        const SpecKernel sp = !linear ? lookup(r0.adapter_lo, r0.adapter_hi, est_cells) : SpecKernel{nullptr, 0};
        const size_t n = e - i;
        if (!sp.spec) {
            if (!out.empty() && !out.back().spec && out.back().begin + out.back().count == i && out.back().chunks == group_chunks)
                out.back().count += n;                       // runs of pairs without a kernel share a launch
            else
                out.push_back({i, n, group_chunks, 0, nullptr, 0, r0.adapter_lo, r0.adapter_hi});
        } else {
            size_t head = n;
            int tail_chunks = 1;
            const size_t slots = (size_t)p.ncu * (size_t)sp.blocks_per_cu;
            // the job's records are [out0, out0 + pairs): its chunked tail gets a region of that many [pair][chunk]
            // entries (not one sized for the whole call: 98 barcode jobs x 245 M pairs would be terabytes), and only
            // while the tails of the call stay within kTailBudget -- later jobs then run whole tiles to the end
            int64_t job_out0 = r0.out0, job_pairs = 0;
            for (size_t q = ri; q < re; ++q) {
                job_out0 = std::min<int64_t>(job_out0, g.runs[q].out0);
                job_pairs = std::max<int64_t>(job_pairs, g.runs[q].out0 + (g.runs[q].dual ? 2 : 1) * g.runs[q].n);
            }
            job_pairs -= job_out0;
            constexpr size_t kTailBudget = (size_t)6 << 30;
            if (group_chunks == 1 && n > slots && n % slots && (k1 + (size_t)job_pairs * 4 * 8) * 4 <= kTailBudget + (size_t)npairs * 16) {
                const size_t tail = n % slots;
                double best = 1.0;                           // in tile-times: one more round of whole tiles
                const double span = 0.5 * g.max_window;
                for (int cc = 2; cc <= 8; ++cc) {
                    if (max_len / cc < std::max(128, g.max_window / 2)) break;
                    const double rounds = (double)((tail * (size_t)cc + slots - 1) / slots);
                    const double cost = rounds / cc * (1.0 + cc * span / std::max(1, max_len));
                    if (cost < best - 0.05) { best = cost; tail_chunks = cc; }
                }
                if (tail_chunks > 1) head = n - tail;
            }
            out.push_back({i, head, group_chunks, 0, sp.spec, sp.blocks_per_cu, r0.adapter_lo, r0.adapter_hi});
            if (head < n) {
                out.push_back({i + head, n - head, tail_chunks, (int64_t)k1 - job_out0 * 4 * tail_chunks, sp.spec, sp.blocks_per_cu,
                               r0.adapter_lo, r0.adapter_hi});
                k1 += (size_t)job_pairs * 4 * (size_t)tail_chunks;
            }
        }
        ri = re;
    }
    if (k1_ints_needed) *k1_ints_needed = k1;
    return out;
}

// ---- ordered and floored second passes -----------------------------------------------------------------------------

// The score floors of a pc_scan_device_floored call: per job, for its first and its second adapter; null: none.
// rule_side: the sides of a pc_scan_device_end_rule call instead, per job (0: start windows, 1: end windows, < 0: the rule
// does not apply to this job); null: no rule.  A call has floors or a rule, never both.
struct Floors { const int32_t *a = nullptr, *b = nullptr, *rule_side = nullptr; };

// PC_MODE_TRACE_AT (the traced minority of a pruned phase B), where the end cells are the caller's: the pairs of each
// segment are taken by end column (coarsely), so that a tile is as long as its latest end cell needs, and every pair traces
// only the columns its path can occupy (plan_kernel).  PC_NO_END_ORDER=1: the pairs as handed over.  (The same scheme over
// PC_MODE_TRACE end windows, behind a score-only pass of the traced kernel, did not pay: profiles/r06_two_pass_ends.txt.)
inline bool ordered_trace_at(const Params &p, const Group &g, int mode)
{
    return !p.opt.no_end_order && mode == PC_MODE_TRACE_AT && g.two_pass && g.rows > 0 && g.nseg > 0 && trace16_plan(p, g.rows, g.max_window + 1);
}

// A floored PC_MODE_TWO_PASS call (pc_scan_device_floored): between the passes the pairs whose best score is below their job's
// floor are answered by the planner ("no alignment") and put behind the others of their segment, by the same bucket pass, so
// that pass 2 costs what the remaining pairs cost: its tiles hold them densely and the tiles behind them end at once.  The
// first pass then leaves score records in d_out -- the specialised kernel writes them itself where a window is one unit --
// which is where the bucket pass and the planner read the end cells, as in PC_MODE_TRACE_AT.  A group none of whose jobs
// has a floor (INT32_MIN) runs exactly as in an unfloored call.
inline int32_t seg_floor_of(const Group &g, size_t s, const Floors &f)
{
    const int32_t sj = g.seg_job[s];
    const int32_t *fl = (sj & 1) ? f.b : f.a;
    return fl ? fl[sj >> 1] : INT32_MIN;
}
inline bool floored(const Group &g, int mode, const Floors &f)
{
    if (!(f.a || f.b) || mode != PC_MODE_TWO_PASS || !g.two_pass || g.nseg == 0 || g.nseg > (size_t)pck::kFloorSegments ||
        g.seg_job.size() != g.nseg)
        return false;
    for (size_t s = 0; s < g.nseg; ++s) if (seg_floor_of(g, s, f) != INT32_MIN) return true;
    return false;
}
// The score pass of a floored group may skip the adapter rows no alignment that reaches its floor can reach (pcb::row_skip_plan;
// the specialised packed-fp16 kernel only).  A launch scans one adapter per half for every job that names it, so its floor for
// adapter `ad` is the lowest floor of those jobs, and INT32_MIN -- no skipping -- as soon as one of them has none.  Not for a
// ruled group (its test is not a plain floor), nor for PC_MODE_SCORE or an unfloored call, which return true scores.
inline int32_t launch_floor(const int32_t *job_adapter, const int32_t *job_adapter_b, int njobs, const Floors &f, int ad)
{
    int64_t lowest = INT64_MAX;
    for (int j = 0; j < njobs; ++j) {
        if (job_adapter[j] == ad) lowest = std::min<int64_t>(lowest, f.a ? f.a[j] : INT32_MIN);
        if (job_adapter_b && job_adapter_b[j] == ad) lowest = std::min<int64_t>(lowest, f.b ? f.b[j] : INT32_MIN);
    }
    return lowest == INT64_MAX ? INT32_MIN : (int32_t)lowest;
}
// Not where the caller asked for none in under-filled launches (PC_SCAN_NO_SKIP_UNDERFILLED, per call) and the fill rule cut
// the group's windows into column chunks (group_chunks: what group_chunks_for returned): a launch of few, short units pays a
// stretch's first window and the LDS round trip of the lower rows at every unit's entry and exit, which on the mask rounds of
// the middle scan cost twice what the skipped rows saved (profiles/mask_rule_before_after.txt).  A launch that fills the chip
// (one chunk) keeps the skip whatever the caller asked.
inline bool row_skip_allowed(const Params &p, const Group &g, int mode, const Floors &f, bool no_skip_underfilled = false, int group_chunks = 1)
{
    if (no_skip_underfilled && group_chunks > 1) return false;
    return !p.opt.no_row_skip && !f.rule_side && floored(g, mode, f);
}

// A call with an end rule (pc_scan_device_end_rule) takes the same route with another test: between the passes the pairs of
// which pc_end_rule.h proves, from their score records and window lengths, that they cannot trim their read are answered by
// the planner and put behind the others.  The windows are short (end windows, 150 columns), so pass 2 is what PC_MODE_TRACE_AT
// runs: pairs by end column, traced windows no longer than the windows themselves.  A group of more than pck::kRuleSegments
// segments, or none of whose jobs has a side, is traced in full.
inline int32_t seg_side_of(const Group &g, size_t s, const Floors &f) { return f.rule_side ? f.rule_side[g.seg_job[s] >> 1] : -1; }
inline bool ruled(const Params &p, const Group &g, int mode, const Floors &f)
{
    if (!p.end_rule || !f.rule_side || (mode != PC_MODE_TWO_PASS && mode != PC_MODE_AUTO) || !g.two_pass || g.nseg == 0 ||
        g.nseg > (size_t)pck::kRuleSegments || g.seg_job.size() != g.nseg || g.seg_win.size() != g.nseg || g.seg_adapter.size() != g.nseg)
        return false;
    for (size_t s = 0; s < g.nseg; ++s) if (seg_side_of(g, s, f) >= 0) return true;
    return false;
}
// segments up to the last one of an ordered (or floored, or ruled) group: the stride of the bucket counters; 0: no such group
inline size_t ordered_segments(const Params &p, const std::vector<Group> &groups, int mode, const Floors &f, bool *any_floored)
{
    size_t n = 0;
    *any_floored = false;
    for (const Group &g : groups) {
        const bool fl = floored(g, mode, f) || ruled(p, g, mode, f);
        *any_floored |= fl;
        if (fl || ordered_trace_at(p, g, mode)) n = std::max(n, g.seg_begin + g.nseg);
    }
    return n;
}

}  // namespace pcn
