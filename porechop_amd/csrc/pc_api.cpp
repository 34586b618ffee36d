// pc_api.cpp -- host side of the C ABI declared in include/porechop_amd.h.
//
// Everything here is plumbing around the kernels in pc_kernels.hip: device buffers, grouping
// pairs into single-adapter tiles, launch order of the two-pass whole-read scan, result
// formatting (porechop/src/alignment.cpp:113-121) and the prefetch memo that turns the
// reference's one-pair-per-call symbol (porechop/src/adapter_align.cpp:11) into a lookup.
// There is deliberately no CPU implementation of the alignment in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <cmath>

#include "../../include/porechop_amd.h"
#include "pc_bounds.h"
#include "pc_slow.h"
#include "pc_paths.h"
#include "pc_umi.h"
#include "pc_umi_dist.h"
#include "pc_consensus.h"
#include "pc_middle_paths.h"
#include "pc_jit.h"
#include "pc_kernels.h"
#include "pc_mask_rule.h"
#include "pc_prefilter_plan.h"
#include "pc_scan_plan.h"

#define PC_VERSION "porechop_amd 0.1 (gfx950)"

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return PC_OK;
        if (p) { if (hipFree(p) != hipSuccess) return PC_ERR_NO_DEVICE; p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&p, want) != hipSuccess) {
            fprintf(stderr, "porechop_amd: hipMalloc(%zu) failed\n", want);
            return PC_ERR_NO_DEVICE;
        }
        cap = want;
        return PC_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return (T *)p; }
};

struct PinBuf {            // page-locked host staging: an async upload from it needs no wait for "the copy has left"
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return PC_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 4 + 256;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return PC_ERR_NO_DEVICE;
        cap = want;
        return PC_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct pc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int ncu = 256;
    int match = 3, mismatch = -6, gap_open = -5, gap_extend = -2;
    std::vector<std::string> adapters;
    std::vector<int> ad_len, ad_window, ad_span;
    bool wildcards = false;                  // pc_set_wildcards: adapter letters are IUPAC sets (pc_letters.h)
    bool wild_packed = false;                // upload_panel: wildcards are on AND the scheme fits scan_kernel's wildcard compare, so the
                                             // launches of this context take the wildcard variants; otherwise the plain ones (the
                                             // degenerate adapters then run the plain-int32 kernel, the others are exact as they are)
    bool panel_dirty = true;
    DevBuf d_ad_codes, d_ad_sets, d_ad_len, d_ad_window, d_ad_span;    // d_ad_sets: d_ad_codes' layout, pcl::letter_set per row
    DevBuf d_slab, d_fin, d_k1, d_woff2, d_wlen2, d_col0, d_ntot, d_frow, d_fscore, d_tcols, d_perm, d_bucket_cnt, d_bucket_slot[2], d_err;
    // the tile table lives in one of two slots: a new table is built (on the context's own stream) in the slot
    // the scans two tables ago used, so building never waits for the scans in flight on the current one
    DevBuf d_tiles_slot[2], d_runs_slot[2];
    PinBuf h_table_slot[2];                          // the run table / segment table of the slot on their way up
    hipEvent_t table_up[2] = {nullptr, nullptr};     // recorded on the context's stream behind those uploads: the staging is free again
    hipEvent_t slot_free[2] = {nullptr, nullptr};    // recorded on the caller's stream after the last launch that reads the slot
    hipEvent_t table_ready = nullptr;                // recorded on the context's stream after the expansion kernel
    int slot = 0;
    // single-pass traced groups of one call (the row classes of phase A / phase B) run two at a time, every
    // other one on the context's own stream, each with its own region of the slab: the tail of one launch
    // is filled by the next.  (No further streams: HIP maps streams onto four hardware queues, and a fifth stream
    // shared a queue with -- and serialised behind -- a caller's upload stream: the record is named in DESIGN.md section 3.)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // host-API staging
    DevBuf d_arena, d_woff, d_wlen, d_out;
    // pc_consensus_round: a slice's trace and votes, the call's per-group tables
    DevBuf d_cons_trace, d_cons_votes, d_cons_meta;
    // pc_phase_b_reduce: job / bin tables in two slots (pinned host staging + device copy each); a slot is reused
    // once the reduce kernel that read it two calls ago has finished (red_done), so a call never waits for the
    // scan it was enqueued behind
    DevBuf d_red_slot[2];
    void *h_red[2] = {nullptr, nullptr};
    size_t h_red_cap[2] = {0, 0};
    hipEvent_t red_done[2] = {nullptr, nullptr};
    int red_slot = 0;
    // score pass: one work counter per launch (units beyond the grid are drawn from it)
    DevBuf d_work;
    DevBuf d_units;              // unit_prefix tables of the launches whose windows are cut into more than kMaxChunks chunks
    int len_hint = 0;            // pc_set_length_hint
    bool int16_only = false;     // pc_set_int16_only: never use the packed-fp16 kernel variants
    bool row_skip_debug = false; // pc_set_row_skip_debug: the row-skipping score launches count their column pairs
    // the prefilter: the plan (pc_prefilter_plan.h) of the last (adapter list, edit bounds, route), its tables on the device
    struct PfCache {
        std::vector<int32_t> key;            // adapters..., max_edits..., route, wildcards; empty: the device holds no plan
        pcp::Plan plan;
    } pf;
    DevBuf d_pf_tables, d_pf_meta;           // exhaustive kernel: Eq tables + piece metadata
    // seed stage (pc_prefilter.hip seed_scan_kernel / seed_verify_kernel): bitmaps, q-gram -> entry ranges, entries,
    // the seeded pieces' metadata and Eq words; candidate list and its counter
    DevBuf d_sd_bitmaps, d_sd_first, d_sd_entries, d_sd_meta, d_sd_eq, d_sd_cand, d_sd_count;
    unsigned long long *h_sd_count = nullptr;   // pinned host copy of the candidate count
    bool pf_defer_count = false;                // pc_prefilter_defer_count: no host round trip inside the prefilter
    int64_t pf_deferred_cap = 0;                // > 0: the last prefilter call left its count check to pc_prefilter_overflowed
    // cached job table (bench loops repeat the same one: skip the re-upload).  The tile table itself only
    // exists on the device: it is expanded there from the groups' runs (one per job and shape).
    pcn::Table table;                        // the plan of the last job list (pc_scan_plan.h): groups, plain-int32 jobs, total
    bool slow_scheme = false;                // the scoring scheme itself is outside the packed kernels' exact range
    std::vector<char> ad_slow;               // per adapter: takes the plain-int32 kernel
    std::vector<int64_t> slow_ad_off;        // offsets of the adapters' letter sets (one byte per row) in d_slow_ad
    DevBuf d_slow_ad, d_slow_state, d_slow_trace;
    DevBuf d_paths_trace;                    // pc_align_paths: the packed trace of one launch (pc_paths.hip)
    DevBuf d_middle_paths_trace;             // pc_middle_paths: the same for its windows, a buffer of its own
    DevBuf d_umi_ops;                        // pc_umi_extract: the operations of one launch (its trace is d_paths_trace)
    std::vector<int32_t> last_job_adapter, last_job_adapter_b;
    std::vector<int64_t> last_job_start;
    int last_max_len = -1, last_mode = -1;
    bool last_end_rule = false;
    bool tiles_uploaded = false;
    std::mutex mu;
    // optional per-launch HIP-event timing (pc_set_timing / pc_get_timing)
    bool timing = false;
    size_t bucket_blocks_at = 0;         // byte offset of the BucketBlock table in d_bucket_slot (behind the segments' first slots)
    struct Timed { hipEvent_t e0, e1; int kind; int64_t pairs; };
    std::vector<Timed> timed;
};

namespace {

using pcp::dna5;

#define HIP_TRY(x)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "porechop_amd: %s failed: %s\n", #x, hipGetErrorString(e_));        \
            return PC_ERR_NO_DEVICE;                                                            \
        }                                                                                       \
    } while (0)

int upload_panel(pc_ctx *c)
{
    if (!c->panel_dirty) return PC_OK;
    const int n = (int)c->adapters.size();
    std::vector<uint32_t> codes((size_t)std::max(n, 1) * pcb::MAX_ADAPTER, 5u);
    std::vector<uint32_t> sets(codes.size(), 0u);
    c->ad_len.assign(std::max(n, 1), 0);
    c->ad_window.assign(std::max(n, 1), 0);
    c->ad_span.assign(std::max(n, 1), 0);
    int maxm = 1;
    // Adapters above pcb::MAX_ADAPTER bases, and every adapter under a scheme outside the packed kernels' exact range,
    // take the plain-int32 kernel (pc_slow.hip): the reference accepts any adapter and any four integers.  With wildcards on the
    // packed kernels read the adapters as sets (trace16_kernel's table, scan_kernel's wildcard variants: pc_kernels.hip); the
    // variants' compare needs 2^kWildShift >= max(match - mismatch, match), and under a scheme beyond that an adapter with a
    // letter the mode reads differently (anything but A/C/G/T/U) takes the plain-int32 kernel too.
    int wild_slow = 0;
    std::vector<char> wild(std::max(n, 1), 0);        // per adapter: it holds a letter the mode reads differently
    const bool wild_fits = std::max((long long)c->match - c->mismatch, (long long)c->match) <= (1ll << pck::kWildShiftHost);
    c->wild_packed = c->wildcards && wild_fits;
    c->ad_slow.assign(std::max(n, 1), 0);
    c->slow_ad_off.assign(std::max(n, 1) + 1, 0);
    std::vector<uint8_t> raw;
    for (int i = 0; i < n; ++i) {
        const std::string &s = c->adapters[i];
        if ((int)s.size() > pcs::MAX_ADAPTER) return PC_ERR_ADAPTER_TOO_LONG;
        c->ad_len[i] = (int)s.size();
        c->slow_ad_off[i] = (int64_t)raw.size();
        bool degenerate = false;
        for (char ch : s) {
            raw.push_back((uint8_t)pcl::letter_set((uint8_t)ch, c->wildcards));
            degenerate |= c->wildcards && pcl::degenerate((uint8_t)ch);
        }
        if (degenerate) wild[i] = 1;
        if (degenerate && !wild_fits) { c->ad_slow[i] = 1; ++wild_slow; }
        if ((int)s.size() > pcb::MAX_ADAPTER) { c->ad_slow[i] = 1; continue; }
        maxm = std::max(maxm, (int)s.size());
        for (size_t k = 0; k < s.size(); ++k) {
            codes[(size_t)i * pcb::MAX_ADAPTER + k] = (uint32_t)dna5((unsigned char)s[k]);
            sets[(size_t)i * pcb::MAX_ADAPTER + k] = pcl::letter_set((uint8_t)s[k], c->wildcards);
        }
    }
    c->slow_ad_off[std::max(n, 1)] = (int64_t)raw.size();
    if (!pcs::fits(0, 0, c->match, c->mismatch, c->gap_open, c->gap_extend)) return PC_ERR_UNSUPPORTED_SCORES;
    c->slow_scheme = !pcb::scores_supported(c->match, c->mismatch, c->gap_open, c->gap_extend, maxm);
    for (int i = 0; i < n; ++i) {
        pcb::Bounds b;
        if (c->slow_scheme || c->ad_slow[i] ||
            !pcb::compute_bounds(c->match, c->mismatch, c->gap_open, c->gap_extend, std::max(1, c->ad_len[i]), b)) {
            c->ad_slow[i] = 1;
            c->ad_window[i] = 0; c->ad_span[i] = 0;
            continue;
        }
        c->ad_window[i] = b.window;
        c->ad_span[i] = b.SPAN;
    }
    {
        // said once per process and cause: the answers are the reference's either way, but a user should know that the run left the
        // fast kernels (PC_QUIET=1 silences it)
        static bool told_scheme = false, told_adapter = false, told_wild = false;
        static const bool quiet = [] { const char *e = getenv("PC_QUIET"); return e && *e && *e != '0'; }();
        int longest_slow = 0;
        for (int i = 0; i < n; ++i)
            if (c->ad_slow[i] && !c->slow_scheme && (!wild[i] || c->ad_len[i] > pcb::MAX_ADAPTER)) longest_slow = std::max(longest_slow, c->ad_len[i]);
        if (wild_slow > 0 && !c->slow_scheme && !told_wild && !quiet) {
            told_wild = true;
            fprintf(stderr, "porechop_amd: wildcards are on and match - mismatch = %d is beyond what the packed kernels' wildcard compare holds "
                            "(%d): the alignments of the %d adapter(s) with letters other than A/C/G/T/U run the plain-int32 kernel -- the same "
                            "answers, roughly a hundred times slower per cell, and none of the exact prunings\n",
                    c->match - c->mismatch, 1 << pck::kWildShiftHost, wild_slow);
        }
        if (c->slow_scheme && n > 0 && !told_scheme && !quiet) {
            told_scheme = true;
            fprintf(stderr, "porechop_amd: scoring scheme %d,%d,%d,%d is outside the packed 16-bit kernels' exact range (they need match > 0, "
                            "match > mismatch, negative gap scores and magnitudes that fit their lanes): every alignment runs the plain-int32 "
                            "kernel -- the same answers, roughly a hundred times slower per cell, and none of the exact prunings\n",
                    c->match, c->mismatch, c->gap_open, c->gap_extend);
        }
        if (longest_slow > 0 && !told_adapter && !quiet) {
            told_adapter = true;
            fprintf(stderr, "porechop_amd: an adapter of %d bases is longer than the %d the packed 16-bit kernels keep in registers: its "
                            "alignments run the plain-int32 kernel (the same answers, roughly a hundred times slower per cell)\n",
                    longest_slow, pcb::MAX_ADAPTER);
        }
    }
    // stream-ordered: earlier launches may still read the old tables
    // the tables below may be in use by scans in flight on ANY stream (callers pass their own): drain the device.
    // (Only when the panel or the scores change.)
    HIP_TRY(hipDeviceSynchronize());
    int rc;
    if ((rc = c->d_ad_codes.ensure(codes.size() * 4)) || (rc = c->d_ad_sets.ensure(sets.size() * 4)) || (rc = c->d_ad_len.ensure(c->ad_len.size() * 4)) ||
        (rc = c->d_ad_window.ensure(c->ad_window.size() * 4)) || (rc = c->d_ad_span.ensure(c->ad_span.size() * 4)))
        return rc;
    HIP_TRY(hipMemcpy(c->d_ad_codes.p, codes.data(), codes.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_ad_sets.p, sets.data(), sets.size() * 4, hipMemcpyHostToDevice));
    if ((rc = c->d_slow_ad.ensure(raw.size() + 16))) return rc;
    if (!raw.empty()) HIP_TRY(hipMemcpy(c->d_slow_ad.p, raw.data(), raw.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_ad_len.p, c->ad_len.data(), c->ad_len.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_ad_window.p, c->ad_window.data(), c->ad_window.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_ad_span.p, c->ad_span.data(), c->ad_span.size() * 4, hipMemcpyHostToDevice));
    c->panel_dirty = false;
    c->pf.key.clear();
    c->tiles_uploaded = false;
    c->last_max_len = -1;
    return PC_OK;
}

// The scan's environment switches, all read here, once per process -- except PC_FORCE_CHUNKS, PC_NO_SCORE_FORK,
// PC_NO_END_FLOOR and PC_NO_ROW_SKIP, which are read for every call (tests change them between calls).
pcn::Options scan_options()
{
    static const pcn::Options once = [] {
        auto on = [](const char *name) { const char *e = getenv(name); return e && *e && *e != '0'; };
        pcn::Options o;
        o.no_split_dual = on("PC_NO_SPLIT_DUAL");
        o.no_merge_small = on("PC_NO_MERGE_SMALL");
        o.f16_disabled = on("PC_DISABLE_F16");
        o.no_trace_fork = on("PC_NO_TRACE_FORK");     // (a profile whose per-kernel durations add up to the step)
        o.no_end_order = on("PC_NO_END_ORDER");
        o.no_pair_trace_bound = on("PC_NO_PAIR_TRACE_BOUND");
        return o;
    }();
    pcn::Options o = once;
    if (const char *f = getenv("PC_FORCE_CHUNKS")) o.force_chunks = atoi(f);
    o.no_score_fork = getenv("PC_NO_SCORE_FORK") != nullptr;
    if (const char *e = getenv("PC_NO_END_FLOOR")) o.no_end_floor = *e && *e != '0';
    if (const char *e = getenv("PC_NO_ROW_SKIP")) o.no_row_skip = *e && *e != '0';
    return o;
}

pcn::Params plan_params(const pc_ctx *c)
{
    pcn::Params p;
    p.ncu = c->ncu; p.len_hint = c->len_hint; p.int16_only = c->int16_only;
    p.match = c->match; p.mismatch = c->mismatch; p.gap_open = c->gap_open; p.gap_extend = c->gap_extend;
    p.opt = scan_options();
    return p;
}

// Build (or reuse) the tile table for a job list: the plan is pcn::build_table's (the jobs' contract is stated there), the
// tile table itself is expanded from the plan's runs on the device.
int build_tiles(pc_ctx *c, const pcn::Params &p, const int32_t *job_adapter, const int32_t *job_adapter_b, const int64_t *job_start,
                int njobs, int max_len, int mode)
{
    std::vector<int32_t> jb(njobs, -1);
    if (job_adapter_b) jb.assign(job_adapter_b, job_adapter_b + njobs);
    const bool same = c->tiles_uploaded && c->last_max_len == max_len && c->last_mode == mode && c->last_end_rule == p.end_rule &&
                      (int)c->last_job_adapter.size() == njobs &&
                      std::equal(job_adapter, job_adapter + njobs, c->last_job_adapter.begin()) &&
                      jb == c->last_job_adapter_b &&
                      std::equal(job_start, job_start + njobs + 1, c->last_job_start.begin());
    if (same) return PC_OK;

    pcn::Table plan;
    const pcn::Panel panel{(int)c->adapters.size(), c->ad_len.data(), c->ad_window.data(), c->ad_slow.data()};
    int rc = pcn::build_table(panel, p, job_adapter, jb.data(), job_start, njobs, max_len, mode, plan);
    if (rc) return rc;
    // from here on the cached table is being replaced: an error below must not leave the "same job list" fast
    // path pointing at half-built groups or an unbuilt slot
    c->tiles_uploaded = false;
    c->last_max_len = -1;
    c->table = std::move(plan);
    const pcn::Table &t = c->table;
    // Build in the other slot: the scans that read it were enqueued two tables ago (their end is marked by
    // slot_free); the scans in flight on the current slot are not waited for.  No device-wide synchronisation:
    // a caller's upload of the next batch on another stream keeps running.
    c->slot ^= 1;
    const int sl = c->slot;
    HIP_TRY(hipEventSynchronize(c->slot_free[sl]));
    HIP_TRY(hipEventSynchronize(c->table_up[sl]));   // (two tables ago: long past)
    rc = c->d_tiles_slot[sl].ensure(std::max<size_t>(1, t.ntiles) * sizeof(pck::Tile));
    if (rc) return rc;
    if ((rc = c->d_runs_slot[sl].ensure(std::max<size_t>(1, t.runs.size()) * sizeof(pck::TileRun)))) return rc;
    c->bucket_blocks_at = (t.seg_first.size() * 8 + 15) & ~(size_t)15;
    if ((rc = c->d_bucket_slot[sl].ensure(c->bucket_blocks_at + std::max<size_t>(1, t.blocks.size()) * sizeof(pck::BucketBlock)))) return rc;
    if (t.ntiles) {
        // The tables go up from page-locked memory of the slot (reusable once table_up[sl] has passed, above): the call does not
        // wait for its own upload -- with the tables in locals it had to, and that wait was for EVERYTHING on the context's
        // stream, the previous call's forked launches among them.
        const size_t seg_bytes = t.seg_first.size() * 8, blk_bytes = t.blocks.size() * sizeof(pck::BucketBlock), run_bytes = t.runs.size() * sizeof(pck::TileRun);
        const size_t blk_at = (seg_bytes + 15) & ~(size_t)15, run_at = (blk_at + blk_bytes + 15) & ~(size_t)15;
        if ((rc = c->h_table_slot[sl].ensure(run_at + run_bytes))) return rc;
        char *hp = (char *)c->h_table_slot[sl].p;
        if (!t.seg_first.empty()) {
            memcpy(hp, t.seg_first.data(), seg_bytes);
            memcpy(hp + blk_at, t.blocks.data(), blk_bytes);
            HIP_TRY(hipMemcpyAsync(c->d_bucket_slot[sl].p, hp, seg_bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync((char *)c->d_bucket_slot[sl].p + c->bucket_blocks_at, hp + blk_at, blk_bytes, hipMemcpyHostToDevice, c->stream));
        }
        // a few hundred bytes per job cross PCIe; the tiles (56 B per 64..128 windows) are written by the GPU
        memcpy(hp + run_at, t.runs.data(), run_bytes);
        HIP_TRY(hipMemcpyAsync(c->d_runs_slot[sl].p, hp + run_at, run_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->table_up[sl], c->stream));
        if (pck::launch_expand_tiles(c->d_runs_slot[sl].as<pck::TileRun>(), (int)t.runs.size(), c->d_tiles_slot[sl].as<pck::Tile>(),
                                     (int64_t)t.ntiles, c->stream))
            return PC_ERR_NO_DEVICE;
        HIP_TRY(hipEventRecord(c->table_ready, c->stream));
    }
    c->last_job_adapter.assign(job_adapter, job_adapter + njobs);
    c->last_job_adapter_b = jb;
    c->last_job_start.assign(job_start, job_start + njobs + 1);
    c->last_max_len = max_len; c->last_mode = mode; c->last_end_rule = p.end_rule;
    c->tiles_uploaded = true;
    return PC_OK;
}

// pairs below their score floor, as two 64-bit counters behind the error words of d_err (bytes 0..23): those of the last floored
// call, and all since the context was made (pc_floor_skipped)
constexpr size_t kFloorCounterAt = 32;
// behind them (bytes 48..63): the row-skip debug counters (pc_set_row_skip_debug / pc_row_skip_blocks)
constexpr size_t kRowSkipCounterAt = 48;

// HIP-event timing of a region of launches (pc_set_timing / pc_get_timing): begin() records on the stream where the region
// starts, end() where it ends, and files the pair under its kind.  c_ == null: untimed.
struct TimedRegion {
    pc_ctx *c = nullptr; hipStream_t s = nullptr; bool on = false; pc_ctx::Timed t;
    void begin(pc_ctx *c_, hipStream_t s_, int kind, int64_t pairs)
    {
        c = c_; s = s_; on = c_ && c_->timing;
        if (!on) return;
        t.kind = kind; t.pairs = pairs;
        if (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(t.e0, s);
    }
    void end() { if (on) { (void)hipEventRecord(t.e1, s); c->timed.push_back(t); on = false; } }
};
struct ScopedTimer : TimedRegion {
    ScopedTimer(pc_ctx *c_, hipStream_t s_, int kind, int64_t pairs) { begin(c_, s_, kind, pairs); }
    ~ScopedTimer() { end(); }
};

int launch_traced(const pcn::Params &p, pck::ScanArgs &a, const pcn::Group &g, int grid, hipStream_t stream)
{
    pcb::F16Plan fp;
    if (pcn::trace16_plan(p, g.rows, a.slab_cols, &fp)) {
        a.f16_cen = fp.cen; a.f16_max_cols = fp.max_cols;
        static const int dbg = [] {
            const char *e = getenv("PC_DEBUG_TRACE"), *r = getenv("PC_CHECK_RANGE");
            return (e ? atoi(e) : 0) | ((r && *r && *r != '0') ? 4 : 0);
        }();
        a.debug = dbg;
        return pck::launch_trace16(a, g.rows, grid, stream);
    }
    return pck::launch_trace(a, g.rows, g.pad, grid, stream);
}

// ---- one scan call: what its steps share ---------------------------------------------------------------------------
struct ScanCall {
    const void *arena; const int64_t *win_off; const int32_t *win_len;      // the caller's reads and windows (device)
    int max_len, mode;
    int32_t *out;
    hipStream_t stream;
    pcn::Floors floors;
    const int32_t *job_adapter = nullptr, *job_adapter_b = nullptr;          // the caller's job list (host), for the launches' floors
    int njobs = 0;
    pcr::EndRule rule;                   // of a call with an end rule (floors.rule_side says for which jobs)
    int64_t npairs;
    bool linear;
    bool no_skip_underfilled = false;    // PC_SCAN_NO_SKIP_UNDERFILLED of this call (pcn::row_skip_allowed)
    // the plan (plan_scan)
    pcn::Params p;
    pcn::Scratch scratch;
    std::vector<std::vector<pcn::ScoreLaunch>> score_plan;       // per group: the launches of its score pass
    size_t k1_ints = 0, n_score_launches = 0;
    size_t unit_ints = 0;                // (real, prefix) tables of the launches cut into very many chunks
    size_t ordered_segments = 0;         // > 0: some group's second pass is ordered or floored (pcn::ordered_segments)
    bool any_floored = false;
    bool fork = false;                   // the single-pass groups alternate between the caller's stream and the context's
    // where the launches are
    size_t unit_at = 0, score_launch_no = 0;
    bool ctx_stream_used = false;
    TimedRegion fork_region;
};

// Everything decided before anything is enqueued: the scratch layout, and the launch plans of the score pass of every two-pass
// group -- they decide how large the pass-1 buffer must be, and growing it later would pull it from under kernels
// already in flight.
void plan_scan(pc_ctx *c, ScanCall &s)
{
    const std::vector<pcn::Group> &groups = c->table.groups;
    s.scratch = pcn::scratch_layout(s.p, groups, s.max_len, s.mode);
    s.fork = s.scratch.n_single >= 2 && s.stream != c->stream && !s.p.opt.no_trace_fork;
    bool skip_ok = false;                // the group being planned may skip rows (pcn::row_skip_allowed)
    auto lookup = [&](int lo, int hi, double cells) {
        // a floored group owes exact records only to pairs that reach their floor: where the pair has the row-skipping kernel
        // and the launch's floors give it thresholds, that one (pc_bounds.h row_skip_plan)
        if (skip_ok) {
            pcj::Spec *sk = pcj::get(c->device, c->adapters[lo], c->adapters[hi], c->match, c->mismatch, c->gap_open, c->gap_extend, cells, c->int16_only, true, c->wildcards);
            pcj::SpecArgs probe;
            if (sk && pcj::row_skip_args(sk, c->match, c->mismatch, c->gap_open, c->gap_extend,
                                         pcn::launch_floor(s.job_adapter, s.job_adapter_b, s.njobs, s.floors, lo),
                                         pcn::launch_floor(s.job_adapter, s.job_adapter_b, s.njobs, s.floors, hi), probe))
                return pcn::SpecKernel{sk, sk->blocks_per_cu};
        }
        pcj::Spec *sp = pcj::get(c->device, c->adapters[lo], c->adapters[hi], c->match, c->mismatch, c->gap_open, c->gap_extend, cells, c->int16_only,
                                 false, c->wildcards);
        return pcn::SpecKernel{sp, sp ? sp->blocks_per_cu : 0};
    };
    s.score_plan.assign(groups.size(), {});
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const pcn::Group &g = groups[gi];
        if (!g.two_pass || s.mode == PC_MODE_TRACE_AT) continue;           // (TRACE_AT: the end cells are the caller's)
        const int group_chunks = pcn::group_chunks_for(s.p, g, s.max_len);
        skip_ok = pcn::row_skip_allowed(s.p, g, s.mode, s.floors, s.no_skip_underfilled, group_chunks);
        size_t need = 0;
        s.score_plan[gi] = pcn::plan_score_launches(s.p, g, s.max_len, s.npairs, group_chunks, lookup, &need);
        s.k1_ints = std::max(s.k1_ints, need);
        s.n_score_launches += s.score_plan[gi].size();
        for (const pcn::ScoreLaunch &L : s.score_plan[gi]) if (L.chunks > pcn::kMaxChunks) s.unit_ints += 2 * (L.count + 1);
    }
    s.ordered_segments = pcn::ordered_segments(s.p, groups, s.mode, s.floors, &s.any_floored);
}

int grow_buffers(pc_ctx *c, const ScanCall &s)
{
    int rc;
    if ((rc = c->d_slab.ensure(s.scratch.slab_bytes + 256)) || (rc = c->d_fin.ensure(s.scratch.fin_bytes + 256))) return rc;
    if (s.n_score_launches) {
        if ((rc = c->d_work.ensure(s.n_score_launches * 4 + 256))) return rc;
        if (s.unit_ints && (rc = c->d_units.ensure(s.unit_ints * 4 + 256))) return rc;
    }
    if (s.ordered_segments &&
        ((rc = c->d_perm.ensure((size_t)s.npairs * 8)) || (rc = c->d_bucket_cnt.ensure(2 * s.ordered_segments * pck::kBucketSlots * 4 + 256))))
        return rc;
    if (s.scratch.any_two) {                       // (an ordered group is a two-pass group)
        const size_t n = (size_t)s.npairs;
        if ((rc = c->d_k1.ensure(s.k1_ints * 4 + 256)) || (rc = c->d_woff2.ensure(n * 8)) || (rc = c->d_wlen2.ensure(n * 4)) ||
            (rc = c->d_col0.ensure(n * 4)) || (rc = c->d_ntot.ensure(n * 4)) || (rc = c->d_frow.ensure(n * 4)) ||
            (rc = c->d_fscore.ensure(n * 4)) || (rc = c->d_tcols.ensure(n * 4)))
            return rc;
    }
    return PC_OK;
}

// Single-pass traced groups of one call run two at a time (see pc_ctx): the fork opens before anything of the call is
// enqueued and closes behind its last launch; the concurrent launches are timed as ONE region.
int open_trace_fork(pc_ctx *c, ScanCall &s)
{
    if (!s.fork) return PC_OK;
    int64_t np_all = 0;
    for (const pcn::Group &g : c->table.groups) if (!g.two_pass) np_all += pcn::group_pairs(g);
    s.fork_region.begin(c, s.stream, 2, np_all);
    HIP_TRY(hipEventRecord(c->ev_fork, s.stream));
    return PC_OK;
}

int close_trace_fork(pc_ctx *c, ScanCall &s)
{
    if (s.ctx_stream_used) {
        HIP_TRY(hipEventRecord(c->ev_join, c->stream));
        HIP_TRY(hipStreamWaitEvent(s.stream, c->ev_join, 0));
    }
    s.fork_region.end();
    return PC_OK;
}

// the work counters of the score launches, the bucket counts and cursors of every ordered group (each group has its own
// rows: one fill) and this call's counter of pairs below their floor
int zero_counters(pc_ctx *c, const ScanCall &s)
{
    if (s.n_score_launches) HIP_TRY(hipMemsetAsync(c->d_work.p, 0, s.n_score_launches * 4, s.stream));
    if (s.ordered_segments) HIP_TRY(hipMemsetAsync(c->d_bucket_cnt.p, 0, 2 * s.ordered_segments * pck::kBucketSlots * 4, s.stream));
    if (s.any_floored || s.p.end_rule) HIP_TRY(hipMemsetAsync((char *)c->d_err.p + kFloorCounterAt, 0, 8, s.stream));
    return PC_OK;
}

// what every launch over group gi is told: the caller's windows, the group's tiles and its scratch regions
pck::ScanArgs group_args(const pc_ctx *c, const ScanCall &s, size_t gi)
{
    const pcn::Group &g = c->table.groups[gi];
    pck::ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.arena = (const uint8_t *)s.arena;
    a.win_off = s.win_off; a.win_len = s.win_len;
    a.ad_codes = c->d_ad_codes.as<uint32_t>();
    a.ad_sets = c->d_ad_sets.as<uint32_t>();
    a.wild = c->wild_packed ? 1 : 0;
    a.ad_len = c->d_ad_len.as<int32_t>();
    a.tiles = c->d_tiles_slot[c->slot].as<pck::Tile>() + g.tile_begin;
    a.ntiles = (int32_t)g.tile_count;
    a.match = c->match; a.mismatch = c->mismatch; a.gap_open = c->gap_open;
    a.gap_extend = s.linear ? pcb::kLinearExtend : c->gap_extend;
    a.init_extend = c->gap_extend; a.linear = s.linear ? 1 : 0;
    a.kren = std::max(1, pcn::drift_period(c->gap_open, c->gap_extend));
    a.err = c->d_err.as<uint32_t>();
    a.slab = (uint32_t *)((char *)c->d_slab.p + s.scratch.slab_off[gi]);
    a.gen_max_rows = g.gen_max_rows;
    a.fin_scratch = (uint32_t *)((char *)c->d_fin.p + s.scratch.fin_off[gi]);
    a.ad_span = c->d_ad_span.as<int32_t>();
    a.ad_window = c->d_ad_window.as<int32_t>();
    return a;
}

// the traced launch of group gi over `slab_cols` columns a window
int run_traced(pc_ctx *c, const ScanCall &s, size_t gi, pck::ScanArgs &a, int slab_cols, pc_ctx *timed, hipStream_t stream)
{
    const pcn::Group &g = c->table.groups[gi];
    size_t stride;
    const int grid = pcn::grid_for(s.p, g, g.tile_count, slab_cols, &stride);
    a.out = s.out;
    a.slab_cols = slab_cols; a.slab_stride = (int64_t)stride;
    ScopedTimer tm(timed, stream, 2, pcn::group_pairs(g));
    return launch_traced(s.p, a, g, grid, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

// The single-pass groups in table order; under the fork every other one on the context's own stream.
int run_single_pass_groups(pc_ctx *c, ScanCall &s)
{
    int n_forked = 0;
    for (size_t gi = 0; gi < c->table.groups.size(); ++gi) {
        if (c->table.groups[gi].two_pass) continue;
        pck::ScanArgs a = group_args(c, s, gi);
        hipStream_t ps = (s.fork && (n_forked++ & 1)) ? c->stream : s.stream;
        if (s.fork && ps == c->stream && !s.ctx_stream_used) { HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_fork, 0)); s.ctx_stream_used = true; }
        const int rc = run_traced(c, s, gi, a, s.max_len, s.fork ? nullptr : c, ps);
        if (rc) return rc;
    }
    return PC_OK;
}

// A two-pass group's first pass, score only over the whole windows: the launches of its plan, each writing its
// [pair][chunk] maxima into its region of the pass-1 buffer.
int score_pass(pc_ctx *c, ScanCall &s, size_t gi, const pck::ScanArgs &a, bool records)
{
    const pcn::Group &g = c->table.groups[gi];
    const std::vector<pcn::ScoreLaunch> &plan = s.score_plan[gi];
    hipStream_t stream = s.stream;
    // A score-only call over short windows (phase B's pruning pass: ~100 launches of 150-column windows, one per
    // adapter pair) cannot cut its tails into column chunks, and every launch would end with a round of tiles that
    // fills a fraction of the chip (15 625 tiles on 3072 resident waves: 15 % of the launch).  Its launches
    // alternate between the caller's stream and the context's: the next kernel's first tiles fill the CUs the
    // previous one's last round leaves idle.  Timed as ONE region.
    const bool ragged = pcn::ragged_lengths(s.p, s.max_len);
    const bool sfork = s.mode == PC_MODE_SCORE && !s.fork && stream != c->stream && plan.size() >= 2 && !ragged &&
                       s.max_len / 2 < std::max(128, g.max_window / 2) && !s.p.opt.no_score_fork;
    bool any_spec = false;
    for (const pcn::ScoreLaunch &L : plan) any_spec |= L.spec != nullptr;
    ScopedTimer region(sfork ? c : nullptr, stream, any_spec ? 3 : 0, pcn::group_pairs(g));
    if (sfork) {
        HIP_TRY(hipEventRecord(c->ev_fork, stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_fork, 0));
    }
    size_t launch_in_group = 0;
    for (const pcn::ScoreLaunch &L : plan) {
        const int chunk_len = (s.max_len + L.chunks - 1) / L.chunks;
        int grid = pcn::grid_for(s.p, g, L.count * (size_t)L.chunks, 1, nullptr);
        const bool alt = sfork && (launch_in_group++ & 1);
        hipStream_t stream_k = alt ? c->stream : stream;
        uint32_t *fin_k = (uint32_t *)((char *)a.fin_scratch + (alt ? s.scratch.fin_region[gi] : 0));
        // windows of very different lengths: exactly the resident workgroups, every further unit drawn from
        // the counter in launch order -- longest first.  (With a larger grid the first workgroups would stay
        // resident drawing the short units while the long ones waited for a slot until the very end.)
        if (ragged)
            grid = (int)std::min<size_t>((size_t)grid, L.spec ? (size_t)c->ncu * (size_t)L.blocks_per_cu : (size_t)pcn::resident_waves(s.p, g));
        ScopedTimer tm(sfork ? nullptr : c, stream, L.spec ? 3 : 0, pcn::group_pairs(g, L.begin, L.begin + L.count));   // one timed region per kernel launch
        // windows cut into very many chunks (a batch with an ultra-long tail): only the chunks that hold columns are units
        const int32_t *unit_prefix = nullptr;
        if (L.chunks > pcn::kMaxChunks) {
            int32_t *real = c->d_units.as<int32_t>() + s.unit_at, *prefix = real + (L.count + 1);
            s.unit_at += 2 * (L.count + 1);
            if (pck::launch_unit_prefix(a.tiles + L.begin, (int)L.count, a.win_len, chunk_len, real, prefix, stream_k)) return PC_ERR_NO_DEVICE;
            unit_prefix = prefix;
        }
        if (L.spec) {
            pcj::SpecArgs sa;
            memset(&sa, 0, sizeof(sa));
            sa.arena = a.arena; sa.win_off = a.win_off; sa.win_len = a.win_len;
            sa.tiles = a.tiles + L.begin; sa.ntiles = (int32_t)L.count;
            sa.out = c->d_k1.as<int32_t>() + L.k1_ints; sa.fin_scratch = fin_k;
            sa.gap_open = c->gap_open; sa.gap_extend = c->gap_extend;
            sa.chunks = L.chunks; sa.chunk_len = chunk_len;
            sa.span = std::max(c->ad_span[L.adapter_lo], c->ad_span[L.adapter_hi]);
            sa.err = a.err;
            sa.work_counter = c->d_work.as<uint32_t>() + s.score_launch_no++;
            // a score-only request over whole windows: the kernel writes the records itself (no planner launch)
            sa.rec_out = (records && L.chunks == 1) ? s.out : nullptr;
            sa.unit_prefix = unit_prefix;
            // the row-skipping kernel -- plan_scan chose it for this launch's floors -- gets its thresholds (pc_bounds.h row_skip_plan)
            if (((const pcj::Spec *)L.spec)->r0 < ((const pcj::Spec *)L.spec)->R) {
                if (!pcj::row_skip_args((const pcj::Spec *)L.spec, c->match, c->mismatch, c->gap_open, c->gap_extend,
                                        pcn::launch_floor(s.job_adapter, s.job_adapter_b, s.njobs, s.floors, L.adapter_lo),
                                        pcn::launch_floor(s.job_adapter, s.job_adapter_b, s.njobs, s.floors, L.adapter_hi), sa))
                    return PC_ERR_BAD_ARG;
                if (c->row_skip_debug) sa.skip_count = (unsigned long long *)((char *)c->d_err.p + kRowSkipCounterAt);
            }
            if (pcj::launch((const pcj::Spec *)L.spec, sa, grid, stream_k)) return PC_ERR_NO_DEVICE;
        } else {
            pck::ScanArgs b = a;
            b.slab = nullptr;
            b.tiles = a.tiles + L.begin; b.ntiles = (int32_t)L.count;
            b.out = c->d_k1.as<int32_t>() + L.k1_ints;
            b.chunks = L.chunks; b.chunk_len = chunk_len;
            b.fin_scratch = fin_k;
            b.work_counter = c->d_work.as<uint32_t>() + s.score_launch_no++;
            b.unit_prefix = unit_prefix;
            if (pck::launch_score(b, g.rows, g.pad, grid, stream_k)) return PC_ERR_NO_DEVICE;
        }
    }
    if (sfork) {
        HIP_TRY(hipEventRecord(c->ev_join, c->stream));
        HIP_TRY(hipStreamWaitEvent(stream, c->ev_join, 0));
    }
    return PC_OK;
}

// Between the passes: the planner turns every pair's best cell into its bounded window (per score launch: the [pair][chunk]
// layout is the launch's); where the end cells are records in the output -- PC_MODE_TRACE_AT, a floored group -- the bucket
// pass orders the pairs first.  Leaves in `a` what pass 2 reads.
int plan_windows(pc_ctx *c, const ScanCall &s, size_t gi, pck::ScanArgs &a, bool fl)
{
    const pcn::Group &g = c->table.groups[gi];
    const bool records = s.mode == PC_MODE_SCORE || fl;
    pck::PlanArgs pl;
    memset(&pl, 0, sizeof(pl));
    pl.win_off = s.win_off; pl.win_len = s.win_len;
    pl.win_off2 = c->d_woff2.as<int64_t>(); pl.win_len2 = c->d_wlen2.as<int32_t>();
    pl.col02 = c->d_col0.as<int32_t>(); pl.ntot2 = c->d_ntot.as<int32_t>();
    pl.force_row2 = c->d_frow.as<int32_t>(); pl.force_score2 = c->d_fscore.as<int32_t>();
    // the pair's own bound on the traced columns (schemes of the packed kernels: match > 0, both gap scores < 0)
    pl.match = c->match; pl.gap_unit = std::min(-c->gap_open, -(s.linear ? c->gap_open : c->gap_extend));
    pl.trace_cols2 = (!s.p.opt.no_pair_trace_bound && pl.match > 0 && pl.gap_unit > 0) ? c->d_tcols.as<int32_t>() : nullptr;
    pl.ad_window = c->d_ad_window.as<int32_t>();
    pl.score_out = records ? s.out : nullptr;
    // end-aligned windows only for the packed-fp16 traced kernel (it is the one that knows lead-ins)
    pl.end_align = pcn::trace16_plan(s.p, g.rows, g.max_window + 1) ? 1 : 0;
    pl.err = a.err;
    // (PC_MODE_TRACE_AT, a call with an end rule: no traced window longer than the windows themselves -- the table's max_window is capped alike)
    if (s.mode == PC_MODE_TRACE_AT || s.p.end_rule) pl.window_cap = std::max(1, s.max_len);
    const bool rl = fl && pcn::ruled(s.p, g, s.mode, s.floors);
    ScopedTimer tm(c, s.stream, 1, pcn::group_pairs(g));
    for (const pcn::ScoreLaunch &L : s.score_plan[gi]) {
        if (records && L.chunks == 1 && L.spec) continue;      // records written by the kernel itself
        pl.k1 = c->d_k1.as<int32_t>() + L.k1_ints;
        pl.tiles = a.tiles + L.begin; pl.ntiles = (int32_t)L.count; pl.chunks = L.chunks;
        pl.chunk_len = (s.max_len + L.chunks - 1) / L.chunks;
        if (pck::launch_plan(pl, s.stream)) return PC_ERR_NO_DEVICE;
    }
    if (s.mode == PC_MODE_TRACE_AT || fl) {   // the score records (the caller's / pass 1's), read before pass 2 overwrites them
        pl.k1 = nullptr; pl.end_records = s.out; pl.score_out = nullptr;
        pl.tiles = a.tiles; pl.ntiles = (int32_t)g.tile_count; pl.chunks = 1;
        if (fl || pcn::ordered_trace_at(s.p, g, s.mode)) {
            pck::BucketArgs b;
            memset(&b, 0, sizeof b);
            b.records = s.out;
            if (fl) {
                b.mark = s.out;
                for (size_t sg = 0; sg < g.nseg; ++sg) b.seg_floor[sg] = rl ? INT32_MIN : pcn::seg_floor_of(g, sg, s.floors);
                if (rl) {
                    b.rule_win_len = s.win_len; b.rule = s.rule;
                    for (size_t sg = 0; sg < g.nseg; ++sg)
                        b.seg_rule[sg] = pck::SegRule{g.seg_win[sg], pcn::seg_side_of(g, sg, s.floors), c->ad_len[g.seg_adapter[sg]]};
                }
                b.skipped = (unsigned long long *)((char *)c->d_err.p + kFloorCounterAt);
                pl.floor_out = s.out;
                a.skip_marked = 1;
            }
            b.seg_first = (const int64_t *)c->d_bucket_slot[c->slot].p + g.seg_begin; b.nsegments = (int32_t)g.nseg;
            b.blocks = (const pck::BucketBlock *)((const char *)c->d_bucket_slot[c->slot].p + c->bucket_blocks_at) + g.blk_begin;
            b.nblocks = (int32_t)g.nblk;
            b.counts = c->d_bucket_cnt.as<uint32_t>() + g.seg_begin * pck::kBucketSlots;
            b.cursors = c->d_bucket_cnt.as<uint32_t>() + (s.ordered_segments + g.seg_begin) * pck::kBucketSlots;
            b.perm = c->d_perm.as<int64_t>();
            if (pck::launch_bucket_pairs(b, s.stream)) return PC_ERR_NO_DEVICE;
            pl.perm = b.perm; a.perm = b.perm;
        }
        if (pck::launch_plan(pl, s.stream)) return PC_ERR_NO_DEVICE;
    }
    // pass 2: traced window ending at the max cell
    a.win_off = pl.win_off2; a.win_len = pl.win_len2; a.col0 = pl.col02; a.n_total = pl.ntot2;
    a.win_by_out = 1;
    a.force_row = pl.force_row2; a.force_score = pl.force_score2; a.trace_cols = pl.trace_cols2;
    a.chunks = 1;
    return PC_OK;
}

int run_two_pass_group(pc_ctx *c, ScanCall &s, size_t gi)
{
    const pcn::Group &g = c->table.groups[gi];
    const bool fl = pcn::floored(g, s.mode, s.floors) || pcn::ruled(s.p, g, s.mode, s.floors);
    pck::ScanArgs a = group_args(c, s, gi);
    int rc;
    if ((rc = score_pass(c, s, gi, a, s.mode == PC_MODE_SCORE || fl))) return rc;
    if ((rc = plan_windows(c, s, gi, a, fl))) return rc;
    if (s.mode == PC_MODE_SCORE) return PC_OK;      // no traceback asked for
    return run_traced(c, s, gi, a, g.max_window + 1, c, s.stream);
}

// jobs outside the packed kernels' range: plain int32, one lane per pair (pc_slow.hip)
int run_slow_jobs(pc_ctx *c, const ScanCall &s)
{
    for (const pcn::SlowJob &J : c->table.slow_jobs) {
        const int m = c->ad_len[J.adapter];
        if (!pcs::fits(s.max_len, m, c->match, c->mismatch, c->gap_open, c->gap_extend)) {
            fprintf(stderr, "porechop_amd: scores %d,%d,%d,%d over windows of up to %d bases and an adapter of %d leave the 32-bit range\n",
                    c->match, c->mismatch, c->gap_open, c->gap_extend, s.max_len, m);
            return PC_ERR_UNSUPPORTED_SCORES;
        }
        static const size_t budget = [] { const char *e = getenv("PC_SLOW_SCRATCH_MB"); return (size_t)(e && atol(e) > 0 ? atol(e) : 2048) << 20; }();
        const bool lds = m <= 128;
        const size_t per_pair = (size_t)std::max(1, s.max_len) * (size_t)m + (lds ? 0 : (size_t)m * 8);
        if ((size_t)pcn::budget_pairs(budget, per_pair) * per_pair > ((size_t)16 << 30)) {
            fprintf(stderr, "porechop_amd: a window of %d bases against an adapter of %d needs %zu bytes of trace per pair: too large for the plain-int32 path\n",
                    s.max_len, m, per_pair);
            return PC_ERR_ADAPTER_TOO_LONG;
        }
        const int64_t P = pcn::slice_pairs(budget, per_pair, J.n);
        int rc;
        if ((rc = c->d_slow_trace.ensure((size_t)P * (size_t)std::max(1, s.max_len) * (size_t)m + 256))) return rc;
        if (!lds && (rc = c->d_slow_state.ensure((size_t)P * (size_t)m * 8 + 256))) return rc;
        pck::SlowArgs sa;
        memset(&sa, 0, sizeof sa);
        sa.arena = (const uint8_t *)s.arena; sa.win_off = s.win_off; sa.win_len = s.win_len;
        sa.adapter = c->d_slow_ad.as<uint8_t>() + c->slow_ad_off[J.adapter];
        sa.m = m; sa.max_len = s.max_len;
        sa.match = c->match; sa.mismatch = c->mismatch; sa.gap_open = c->gap_open; sa.gap_extend = c->gap_extend;
        sa.out = s.out; sa.state = lds ? nullptr : c->d_slow_state.as<int32_t>(); sa.trace = c->d_slow_trace.as<uint8_t>();
        sa.P = P; sa.err = c->d_err.as<uint32_t>();
        ScopedTimer tm(c, s.stream, 2, J.n);
        for (int64_t first = 0; first < J.n; first += P) {
            sa.first_window = J.win_start + first; sa.count = std::min<int64_t>(P, J.n - first); sa.out_base = J.out_base + first;
            if (pck::launch_slow(sa, s.stream)) return PC_ERR_NO_DEVICE;
        }
    }
    return PC_OK;
}

int scan_device(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                int64_t nwindows, const int32_t *job_adapter, const int32_t *job_adapter_b,
                const int64_t *job_start, int njobs, int max_len, int mode, int32_t *d_out, void *stream_v,
                const int32_t *job_floor, const int32_t *job_floor_b, const pc_end_rule *rule = nullptr, const int32_t *job_side = nullptr,
                int flags = 0)
{
    // 1: the arguments, the panel, the table of the job list
    if (!c || nwindows < 0 || njobs < 0 || max_len < 0) return PC_ERR_BAD_ARG;
    if (nwindows == 0 || njobs == 0) return PC_OK;
    if (!d_arena || !d_win_off || !d_win_len || !job_adapter || !job_start || !d_out) return PC_ERR_BAD_ARG;
    if (job_start[0] < 0 || job_start[njobs] > nwindows) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    int rc = upload_panel(c);
    if (rc) return rc;
    ScanCall s;
    s.arena = d_arena; s.win_off = d_win_off; s.win_len = d_win_len; s.max_len = max_len; s.mode = mode; s.out = d_out;
    s.stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    s.floors.a = job_floor; s.floors.b = job_floor_b;
    s.job_adapter = job_adapter; s.job_adapter_b = job_adapter_b; s.njobs = njobs;
    s.linear = pcb::is_linear(c->gap_open, c->gap_extend);
    s.no_skip_underfilled = (flags & PC_SCAN_NO_SKIP_UNDERFILLED) != 0;
    s.p = plan_params(c);
    if (rule && job_side && !s.p.opt.no_end_floor) {
        s.p.end_rule = true;
        s.floors.rule_side = job_side;
        s.rule = pcr::make_end_rule(c->match, c->mismatch, c->gap_open, c->gap_extend, rule->end_size, rule->min_trim_size,
                                    rule->extra_end_trim, rule->end_threshold);
    }
    if ((rc = build_tiles(c, s.p, job_adapter, job_adapter_b, job_start, njobs, max_len, mode))) return rc;
    s.npairs = c->table.total;
    if (mode == PC_MODE_SCORE && !c->table.slow_jobs.empty()) {
        // score-only records (the end cell) feed bounds that are derived for the packed kernels' schemes (pc_select.hip)
        fprintf(stderr, "porechop_amd: PC_MODE_SCORE is not available for scoring schemes / adapters that take the plain-int32 kernel\n");
        return PC_ERR_UNSUPPORTED_SCORES;
    }
    if (s.stream != c->stream) HIP_TRY(hipStreamWaitEvent(s.stream, c->table_ready, 0));   // the table is built on the context's stream
    // 2, 3: the plan of the call, and room for it
    plan_scan(c, s);
    if ((rc = grow_buffers(c, s))) return rc;
    // 4: the single-pass groups, side by side on two streams
    if ((rc = open_trace_fork(c, s)) || (rc = zero_counters(c, s)) || (rc = run_single_pass_groups(c, s))) return rc;
    // 5: the two-pass groups, one after the other
    for (size_t gi = 0; gi < c->table.groups.size(); ++gi)
        if (c->table.groups[gi].two_pass && (rc = run_two_pass_group(c, s, gi))) return rc;
    if ((rc = close_trace_fork(c, s))) return rc;
    // 6, 7: the plain-int32 jobs; the last launch that reads this table slot
    if ((rc = run_slow_jobs(c, s))) return rc;
    HIP_TRY(hipEventRecord(c->slot_free[c->slot], s.stream));
    return PC_OK;
}

}  // namespace

extern "C" {

const char *pc_version(void) { return PC_VERSION; }

const char *pc_strerror(int code)
{
    switch (code) {
        case PC_OK: return "ok";
        case PC_ERR_NO_DEVICE: return "no usable HIP device / HIP runtime error";
        case PC_ERR_UNSUPPORTED_SCORES: return "scores beyond the 32-bit-safe range of the GPU path (|score| <= 2^20; PC_MODE_SCORE needs the packed kernels' schemes)";
        case PC_ERR_BAD_ARG: return "bad argument";
        case PC_ERR_ADAPTER_TOO_LONG: return "adapter longer than PC_MAX_ADAPTER_ANY (or its trace too large)";
        case PC_ERR_INTERNAL: return "kernel reported an internal inconsistency";
        case PC_ERR_OVER_BUDGET: return "one consensus group alone needs more scratch than PC_CONSENSUS_SCRATCH_MB allows";
        default: return "unknown error";
    }
}

int pc_scores_supported(int match, int mismatch, int gap_open, int gap_extend, int max_adapter_len)
{
    if (max_adapter_len > pcb::MAX_ADAPTER) return 0;
    return pcb::scores_supported(match, mismatch, gap_open, gap_extend, std::max(1, max_adapter_len)) ? 1 : 0;
}

int pc_create(pc_ctx **out, int device)
{
    if (!out) return PC_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "porechop_amd: no HIP device visible -- this library has no CPU path\n");
        return PC_ERR_NO_DEVICE;
    }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return PC_ERR_NO_DEVICE; }
    if (device >= ndev) return PC_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(device));
    pc_ctx *c = new pc_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->ncu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
    if (c->d_err.ensure(256) != PC_OK || hipMemset(c->d_err.p, 0, 256) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
    for (int i = 0; i < 2; ++i) {
        if (hipEventCreateWithFlags(&c->slot_free[i], hipEventDisableTiming) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
        if (hipEventCreateWithFlags(&c->table_up[i], hipEventDisableTiming) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
    }
    if (hipEventCreateWithFlags(&c->table_ready, hipEventDisableTiming) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
    for (int i = 0; i < 2; ++i)
        if (hipEventCreateWithFlags(&c->red_done[i], hipEventDisableTiming) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
    if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) { delete c; return PC_ERR_NO_DEVICE; }
    *out = c;
    return PC_OK;
}

void pc_destroy(pc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 2; ++i) if (c->slot_free[i]) (void)hipEventDestroy(c->slot_free[i]);
    for (int i = 0; i < 2; ++i) if (c->table_up[i]) (void)hipEventDestroy(c->table_up[i]);
    if (c->table_ready) (void)hipEventDestroy(c->table_ready);
    for (int i = 0; i < 2; ++i) {
        if (c->red_done[i]) (void)hipEventDestroy(c->red_done[i]);
        if (c->h_red[i]) (void)hipHostFree(c->h_red[i]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    DevBuf *bufs[] = {&c->d_ad_codes, &c->d_ad_sets, &c->d_ad_len, &c->d_ad_window, &c->d_ad_span, &c->d_tiles_slot[0], &c->d_tiles_slot[1],
                      &c->d_runs_slot[0], &c->d_runs_slot[1], &c->d_slab, &c->d_fin, &c->d_k1, &c->d_woff2,
                      &c->d_wlen2, &c->d_col0, &c->d_ntot, &c->d_frow, &c->d_fscore, &c->d_tcols, &c->d_perm, &c->d_bucket_cnt, &c->d_bucket_slot[0], &c->d_bucket_slot[1], &c->d_err, &c->d_arena,
                      &c->d_woff, &c->d_wlen, &c->d_out, &c->d_red_slot[0], &c->d_red_slot[1], &c->d_work, &c->d_units, &c->d_pf_tables, &c->d_pf_meta, &c->d_sd_bitmaps, &c->d_sd_first,
                      &c->d_sd_entries, &c->d_sd_meta, &c->d_sd_eq, &c->d_sd_cand, &c->d_sd_count, &c->d_slow_ad, &c->d_slow_state,
                      &c->d_slow_trace, &c->d_paths_trace, &c->d_middle_paths_trace, &c->d_umi_ops, &c->d_cons_trace, &c->d_cons_votes,
                      &c->d_cons_meta};
    if (c->h_sd_count) (void)hipHostFree(c->h_sd_count);
    c->h_table_slot[0].release(); c->h_table_slot[1].release();
    for (DevBuf *b : bufs) b->release();
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int pc_set_scores(pc_ctx *c, int match, int mismatch, int gap_open, int gap_extend)
{
    if (!c) return PC_ERR_BAD_ARG;
    // any four integers the reference's int arithmetic can hold: schemes outside pcb::scores_supported run the
    // plain-int32 kernel (pc_slow.hip); only magnitudes above 2^20 are refused
    if (!pcs::fits(0, 0, match, mismatch, gap_open, gap_extend)) return PC_ERR_UNSUPPORTED_SCORES;
    if (match != c->match || mismatch != c->mismatch || gap_open != c->gap_open || gap_extend != c->gap_extend) {
        c->match = match; c->mismatch = mismatch; c->gap_open = gap_open; c->gap_extend = gap_extend;
        c->panel_dirty = true;
    }
    return PC_OK;
}

int pc_set_wildcards(pc_ctx *c, int enabled)
{
    if (!c) return PC_ERR_BAD_ARG;
    // everything derived from the panel's letters is redone by the next call (upload_panel: the letter sets, which adapters leave
    // the packed kernels, the tile table; the prefilter plan's key holds the mode itself)
    if ((enabled != 0) != c->wildcards) {
        c->wildcards = enabled != 0;
        c->panel_dirty = true;
    }
    return PC_OK;
}

int pc_letter_set(int byte, int wildcards)
{
    if (byte < 0 || byte > 255) return 0;
    return (int)pcl::letter_set((uint8_t)byte, wildcards != 0);
}

int pc_set_int16_only(pc_ctx *c, int enabled)
{
    if (!c) return PC_ERR_BAD_ARG;
    c->int16_only = enabled != 0;
    return PC_OK;
}

int pc_set_length_hint(pc_ctx *c, int typical_len)
{
    if (!c || typical_len < 0) return PC_ERR_BAD_ARG;
    c->len_hint = typical_len;
    return PC_OK;
}

int pc_set_adapters(pc_ctx *c, const char *const *seqs, int n)
{
    if (!c || n < 0 || (n > 0 && !seqs)) return PC_ERR_BAD_ARG;
    std::vector<std::string> v;
    for (int i = 0; i < n; ++i) {
        if (!seqs[i]) return PC_ERR_BAD_ARG;
        v.emplace_back(seqs[i]);
        if (v.back().size() > (size_t)pcs::MAX_ADAPTER) return PC_ERR_ADAPTER_TOO_LONG;
    }
    c->adapters.swap(v);
    c->panel_dirty = true;
    (void)hipSetDevice(c->device);
    return upload_panel(c);
}

int pc_scan_device(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                   int64_t nwindows, const int32_t *job_adapter, const int32_t *job_adapter_b,
                   const int64_t *job_start, int njobs, int max_len, int mode, int32_t *d_out, void *stream_v)
{
    return scan_device(c, d_arena, d_win_off, d_win_len, nwindows, job_adapter, job_adapter_b, job_start, njobs, max_len, mode, d_out,
                       stream_v, nullptr, nullptr);
}

int pc_scan_device_floored(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                           int64_t nwindows, const int32_t *job_adapter, const int32_t *job_adapter_b,
                           const int64_t *job_start, int njobs, int max_len, int mode, int32_t *d_out, void *stream_v,
                           const int32_t *job_floor, const int32_t *job_floor_b)
{
    if ((job_floor || job_floor_b) && mode != PC_MODE_TWO_PASS) return PC_ERR_BAD_ARG;     // floors sit between the two passes
    if (job_floor_b && !job_adapter_b) return PC_ERR_BAD_ARG;
    return scan_device(c, d_arena, d_win_off, d_win_len, nwindows, job_adapter, job_adapter_b, job_start, njobs, max_len, mode, d_out,
                       stream_v, job_floor, job_floor_b);
}

int pc_scan_device_floored_flags(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                                 int64_t nwindows, const int32_t *job_adapter, const int32_t *job_adapter_b,
                                 const int64_t *job_start, int njobs, int max_len, int mode, int32_t *d_out, void *stream_v,
                                 const int32_t *job_floor, const int32_t *job_floor_b, int flags)
{
    if ((job_floor || job_floor_b) && mode != PC_MODE_TWO_PASS) return PC_ERR_BAD_ARG;
    if (job_floor_b && !job_adapter_b) return PC_ERR_BAD_ARG;
    if (flags & ~PC_SCAN_NO_SKIP_UNDERFILLED) return PC_ERR_BAD_ARG;
    return scan_device(c, d_arena, d_win_off, d_win_len, nwindows, job_adapter, job_adapter_b, job_start, njobs, max_len, mode, d_out,
                       stream_v, job_floor, job_floor_b, nullptr, nullptr, flags);
}

int pc_scan_device_end_rule(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                            int64_t nwindows, const int32_t *job_adapter, const int32_t *job_adapter_b,
                            const int64_t *job_start, int njobs, int max_len, int mode, int32_t *d_out, void *stream_v,
                            const pc_end_rule *rule, const int32_t *job_side)
{
    if ((rule || job_side) && mode != PC_MODE_AUTO && mode != PC_MODE_TWO_PASS) return PC_ERR_BAD_ARG;   // the rule sits between two passes
    if ((rule != nullptr) != (job_side != nullptr)) return PC_ERR_BAD_ARG;
    if (rule && (rule->end_size < 0 || !(rule->end_threshold == rule->end_threshold))) return PC_ERR_BAD_ARG;
    return scan_device(c, d_arena, d_win_off, d_win_len, nwindows, job_adapter, job_adapter_b, job_start, njobs, max_len, mode, d_out,
                       stream_v, nullptr, nullptr, rule, job_side);
}

int pc_floor_skipped(pc_ctx *c, void *stream_v, int64_t *last_call, int64_t *total)
{
    if (!c || (!last_call && !total)) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipStreamSynchronize(stream));
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, (char *)c->d_err.p + kFloorCounterAt, 16, hipMemcpyDeviceToHost));
    if (last_call) *last_call = (int64_t)v[0];
    if (total) *total = (int64_t)v[1];
    return PC_OK;
}


int pc_set_row_skip_debug(pc_ctx *c, int enabled)
{
    if (!c) return PC_ERR_BAD_ARG;
    c->row_skip_debug = enabled != 0;
    return PC_OK;
}

int pc_row_skip_blocks(pc_ctx *c, void *stream_v, int64_t *column_pairs, int64_t *lower_rows_on)
{
    if (!c || (!column_pairs && !lower_rows_on)) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipStreamSynchronize(stream));
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, (char *)c->d_err.p + kRowSkipCounterAt, 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset((char *)c->d_err.p + kRowSkipCounterAt, 0, 16));
    if (column_pairs) *column_pairs = (int64_t)v[0];
    if (lower_rows_on) *lower_rows_on = (int64_t)v[1];
    return PC_OK;
}

int pc_debug_value_range(pc_ctx *c, int32_t *lo, int32_t *hi)
{
    if (!c || !lo || !hi) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    HIP_TRY(hipDeviceSynchronize());
    int32_t v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, (char *)c->d_err.p + 16, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset((char *)c->d_err.p + 16, 0, 8));
    *hi = v[0]; *lo = -v[1];
    return PC_OK;
}

namespace {

// trace scratch one launch of a path kernel may take, unless PC_PATHS_SCRATCH_MB says otherwise
constexpr size_t kPathsScratchMB = 256;

// rows: the table's longest adapter (the LDS rows of both path kernels).  cols: the widest window a MIDDLE hit can have
// over reads of up to max_len bases -- min(max_len, the largest window + W of the table), max_len as soon as one adapter
// takes the whole read (ad_window 0: compute_bounds refused)
int paths_shape(pc_ctx *c, int max_len, int &rows, int &cols)
{
    const int rc = upload_panel(c);
    if (rc) return rc;
    rows = 1;
    int64_t widest = 0;
    for (size_t i = 0; i < c->adapters.size(); ++i) {
        if (c->ad_len[i] > pcb::MAX_ADAPTER) return PC_ERR_BAD_ARG;     // the code table holds 128 bases per adapter
        rows = std::max(rows, c->ad_len[i]);
        const int64_t window = c->ad_window[i], W = window - c->ad_span[i] - 1;
        widest = std::max(widest, window > 0 ? window + W : (int64_t)max_len);
    }
    cols = (int)std::min<int64_t>(max_len, widest);
    return PC_OK;
}

// What pc_align_paths and pc_middle_paths do alike once their own argument checks have passed, for n alignments of up to
// cols columns and rows rows: refuse what leaves int32, size a launch's slice P from the scratch budget (read per call:
// tests force several slices with a few hundred alignments), make `scratch` hold it, fill what `a` takes from the context.
int paths_setup(pc_ctx *c, int cols, int rows, int max_len, int64_t n, DevBuf &scratch, pck::PathArgs &a)
{
    if (!pcs::fits(cols, rows, c->match, c->mismatch, c->gap_open, c->gap_extend)) {
        fprintf(stderr, "porechop_amd: scores %d,%d,%d,%d over windows of up to %d bases and an adapter of %d leave the 32-bit range\n",
                c->match, c->mismatch, c->gap_open, c->gap_extend, cols, rows);
        return PC_ERR_UNSUPPORTED_SCORES;
    }
    size_t budget = kPathsScratchMB << 20;
    if (const char *e = getenv("PC_PATHS_SCRATCH_MB")) { if (atol(e) > 0) budget = (size_t)atol(e) << 20; }
    const int groups = pcpath::row_groups(rows);
    const size_t per_lane = (size_t)std::max(1, cols) * (size_t)groups * 4;
    const int64_t P = pcn::slice_pairs(budget, per_lane, n);
    const int rc = scratch.ensure((size_t)P * per_lane + 256);
    if (rc) return rc;
    a.ad_sets = c->d_ad_sets.as<uint32_t>(); a.ad_len = c->d_ad_len.as<int32_t>(); a.nadapters = (int32_t)c->adapters.size();
    a.rows = rows; a.groups = groups; a.max_len = max_len;
    a.match = c->match; a.mismatch = c->mismatch; a.gap_open = c->gap_open; a.gap_extend = c->gap_extend;
    a.trace = scratch.as<uint32_t>(); a.P = P; a.err = c->d_err.as<uint32_t>();
    return PC_OK;
}

}  // namespace

int pc_align_paths(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                   const int32_t *d_adapter_idx, int64_t n, int max_len, int32_t *d_records, int32_t *d_heads,
                   uint32_t *d_ops, int64_t ops_pitch_words, void *stream_v)
{
    if (!c || n < 0 || max_len < 0 || ops_pitch_words < 0) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    int rows, middle_cols;
    int rc = paths_shape(c, max_len, rows, middle_cols);
    if (rc) return rc;
    if (ops_pitch_words < pcpath::ops_words(max_len, c->adapters.empty() ? 0 : rows)) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_arena || !d_win_off || !d_win_len || !d_adapter_idx || !d_records || !d_heads || !d_ops) return PC_ERR_BAD_ARG;
    pck::PathArgs a{};
    if ((rc = paths_setup(c, max_len, rows, max_len, n, c->d_paths_trace, a))) return rc;
    a.arena = (const uint8_t *)d_arena; a.seq_off = d_win_off; a.seq_len = d_win_len; a.adapter_idx = d_adapter_idx;
    a.records = d_records; a.heads = d_heads; a.ops = d_ops; a.ops_pitch = ops_pitch_words;
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    for (int64_t first = 0; first < n; first += a.P) {
        a.first = first; a.count = std::min<int64_t>(a.P, n - first);
        if (pck::launch_paths(a, stream)) return PC_ERR_NO_DEVICE;
    }
    return PC_OK;
}

int pc_middle_paths_cols(pc_ctx *c, int max_len)
{
    if (!c || max_len < 0) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    int rows, cols;
    const int rc = paths_shape(c, max_len, rows, cols);
    return rc ? rc : cols;
}

int pc_middle_paths(pc_ctx *c, const void *d_arena, const int64_t *d_read_off, const int32_t *d_read_len,
                    const int32_t *d_adapter_idx, const int32_t *d_read_end, const int64_t *d_mask_base,
                    const int32_t *d_mask_count, const int32_t *d_intervals, int64_t n, int max_len,
                    int32_t *d_records, int32_t *d_heads, uint32_t *d_ops, int64_t ops_pitch_words, void *stream_v)
{
    if (!c || n < 0 || max_len < 0 || ops_pitch_words < 0) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    int rows, cols;
    int rc = paths_shape(c, max_len, rows, cols);
    if (rc) return rc;
    if (ops_pitch_words < pcpath::ops_words(cols, c->adapters.empty() ? 0 : rows)) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_arena || !d_read_off || !d_read_len || !d_adapter_idx || !d_read_end || !d_mask_base || !d_mask_count ||
        !d_intervals || !d_records || !d_heads || !d_ops) return PC_ERR_BAD_ARG;
    pck::MiddlePathArgs a{};
    if ((rc = paths_setup(c, cols, rows, max_len, n, c->d_middle_paths_trace, a))) return rc;
    a.arena = (const uint8_t *)d_arena; a.seq_off = d_read_off; a.seq_len = d_read_len; a.adapter_idx = d_adapter_idx;
    a.read_end = d_read_end; a.mask_base = d_mask_base; a.mask_count = d_mask_count; a.intervals = d_intervals; a.n = n;
    a.records = d_records; a.heads = d_heads; a.ops = d_ops; a.ops_pitch = ops_pitch_words;
    a.ad_window = c->d_ad_window.as<int32_t>(); a.ad_span = c->d_ad_span.as<int32_t>(); a.max_cols = cols;
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    for (int64_t first = 0; first < n; first += a.P) {
        a.first = first; a.count = std::min<int64_t>(a.P, n - first);
        if (pck::launch_middle_paths(a, stream)) return PC_ERR_NO_DEVICE;
    }
    return PC_OK;
}

int pc_umi_span(pc_ctx *c, int adapter, int *first, int *last)
{
    if (!c || adapter < 0 || adapter >= (int)c->adapters.size()) return PC_ERR_BAD_ARG;
    const std::string &s = c->adapters[adapter];
    const bool wild = c->wildcards;
    int u0, u1;
    const bool has = pcu::span([&](int k) { return pcl::letter_set((uint8_t)s[k], wild); }, (int)s.size(), &u0, &u1);
    if (first) *first = u0;
    if (last) *last = u1;
    return has ? 1 : 0;
}

int pc_umi_extract(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len, int64_t n,
                   int max_len, int adapter, int side, const pc_end_rule *rule, int32_t *d_records, int32_t *d_umi,
                   void *stream_v)
{
    if (!c || n < 0 || max_len < 0 || side < 0 || side > 1) return PC_ERR_BAD_ARG;
    if (adapter < 0 || adapter >= (int)c->adapters.size() || !c->wildcards) return PC_ERR_BAD_ARG;
    const int m = (int)c->adapters[adapter].size();
    if (m > pcb::MAX_ADAPTER) return PC_ERR_BAD_ARG;                 // the code table holds 128 rows per adapter
    int u0, u1;
    if (pc_umi_span(c, adapter, &u0, &u1) != 1) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    int rc = upload_panel(c);
    if (rc) return rc;
    if (n == 0) return PC_OK;
    if (!d_arena || !d_win_off || !d_win_len || !d_records || !d_umi) return PC_ERR_BAD_ARG;
    if (!pcs::fits(max_len, m, c->match, c->mismatch, c->gap_open, c->gap_extend)) {
        fprintf(stderr, "porechop_amd: scores %d,%d,%d,%d over windows of up to %d bases and an adapter of %d leave the 32-bit range\n",
                c->match, c->mismatch, c->gap_open, c->gap_extend, max_len, m);
        return PC_ERR_UNSUPPORTED_SCORES;
    }
    // pc_align_paths' slicing rule over THIS adapter's rows: a lane's trace and, behind it, its operations
    size_t budget = kPathsScratchMB << 20;
    if (const char *e = getenv("PC_PATHS_SCRATCH_MB")) { if (atol(e) > 0) budget = (size_t)atol(e) << 20; }
    const int groups = pcpath::row_groups(m);
    const int64_t words = std::max<int64_t>(1, pcpath::ops_words(max_len, m));
    const size_t trace_lane = (size_t)std::max(1, max_len) * (size_t)groups * 4;
    const int64_t P = pcn::slice_pairs(budget, trace_lane + (size_t)words * 4, n);
    if ((rc = c->d_paths_trace.ensure((size_t)P * trace_lane + 256))) return rc;
    if ((rc = c->d_umi_ops.ensure((size_t)P * (size_t)words * 4 + 256))) return rc;
    pck::UmiArgs a{};
    a.arena = (const uint8_t *)d_arena; a.win_off = d_win_off; a.win_len = d_win_len;
    a.ad_sets = c->d_ad_sets.as<uint32_t>() + (size_t)adapter * pcb::MAX_ADAPTER;
    a.m = m; a.groups = groups; a.max_len = max_len;
    a.match = c->match; a.mismatch = c->mismatch; a.gap_open = c->gap_open; a.gap_extend = c->gap_extend;
    a.u0 = u0; a.u1 = u1; a.side = side; a.ruled = rule ? 1 : 0;
    if (rule) { a.end_size = rule->end_size; a.min_trim_size = rule->min_trim_size; a.end_threshold = rule->end_threshold; }
    a.records = d_records; a.umi = d_umi;
    a.trace = c->d_paths_trace.as<uint32_t>(); a.ops = c->d_umi_ops.as<uint32_t>(); a.ops_words = words; a.P = P;
    a.err = c->d_err.as<uint32_t>();
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    for (int64_t first = 0; first < n; first += P) {
        a.first = first; a.count = std::min<int64_t>(P, n - first);
        if (pck::launch_umi(a, stream)) return PC_ERR_NO_DEVICE;
    }
    return PC_OK;
}

static int umi_neighbours_call(pc_ctx *c, const uint64_t *d_planes, const int32_t *d_len, int64_t n, int max_len, int max_dist,
                               int32_t *d_pairs, int64_t cap, int64_t *d_found, void *stream_v, bool stranded)
{
    if (!c || !d_found || n < 0 || n > (int64_t)INT32_MAX || cap < 0) return PC_ERR_BAD_ARG;
    if (max_len < 0 || max_len > pcud::MAX_LEN || max_dist < 0 || max_dist > pcud::MAX_LEN) return PC_ERR_BAD_ARG;
    if (n >= 2 && (!d_planes || !d_len || (cap > 0 && !d_pairs))) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_found, 0, sizeof(int64_t), stream));
    if (n < 2) return PC_OK;
    const char *e = getenv("PC_UMI_NO_PRUNE");                       // read per call: the DP for every pair
    pck::UmiNeighboursArgs a{};
    a.planes = d_planes; a.len = d_len; a.n = n; a.max_len = max_len; a.max_dist = max_dist;
    a.prune = (e && atoi(e) != 0) ? 0 : 1;
    a.pairs = d_pairs; a.cap = cap; a.found = (unsigned long long *)d_found;
    a.err = c->d_err.as<uint32_t>();
    if (stranded ? pck::launch_umi_neighbours_stranded(a, stream) : pck::launch_umi_neighbours(a, stream)) return PC_ERR_NO_DEVICE;
    return PC_OK;
}

int pc_umi_neighbours(pc_ctx *c, const uint64_t *d_planes, const int32_t *d_len, int64_t n, int max_len, int max_dist,
                      int32_t *d_pairs, int64_t cap, int64_t *d_found, void *stream_v)
{
    return umi_neighbours_call(c, d_planes, d_len, n, max_len, max_dist, d_pairs, cap, d_found, stream_v, false);
}

int pc_umi_neighbours_stranded(pc_ctx *c, const uint64_t *d_planes, const int32_t *d_len, int64_t n, int max_len, int max_dist,
                               int32_t *d_pairs, int64_t cap, int64_t *d_found, void *stream_v)
{
    return umi_neighbours_call(c, d_planes, d_len, n, max_len, max_dist, d_pairs, cap, d_found, stream_v, true);
}

// votes and trace one slice of pc_consensus_round may take, unless PC_CONSENSUS_SCRATCH_MB says otherwise
static constexpr size_t kConsensusScratchMB = 4096;

int pc_consensus_round(pc_ctx *c, const void *d_arena, const void *d_tmpl_arena, const int64_t *h_tmpl_off, const int32_t *h_tmpl_len,
                       const int64_t *h_group_first, int64_t n_groups, const int64_t *d_member_off, const int32_t *d_member_len,
                       const int32_t *d_member_group, int64_t n_members, int band, int max_err_pct, int max_len, int tmpl_counts,
                       uint8_t *d_cons, int32_t *d_cons_len, int32_t *d_voters, int32_t *d_member_out, uint32_t *d_votes,
                       int64_t *refused_group, void *stream_v)
{
    return pc_consensus_round_stranded(c, d_arena, d_tmpl_arena, h_tmpl_off, h_tmpl_len, h_group_first, n_groups, d_member_off, d_member_len,
                                       d_member_group, nullptr, n_members, band, max_err_pct, max_len, tmpl_counts, d_cons, d_cons_len,
                                       d_voters, d_member_out, d_votes, refused_group, stream_v);
}

int pc_consensus_round_stranded(pc_ctx *c, const void *d_arena, const void *d_tmpl_arena, const int64_t *h_tmpl_off,
                                const int32_t *h_tmpl_len, const int64_t *h_group_first, int64_t n_groups, const int64_t *d_member_off,
                                const int32_t *d_member_len, const int32_t *d_member_group, const uint8_t *d_member_strand,
                                int64_t n_members, int band, int max_err_pct, int max_len, int tmpl_counts, uint8_t *d_cons,
                                int32_t *d_cons_len, int32_t *d_voters, int32_t *d_member_out, uint32_t *d_votes, int64_t *refused_group,
                                void *stream_v)
{
    return pc_consensus_round_quality(c, d_arena, d_tmpl_arena, h_tmpl_off, h_tmpl_len, h_group_first, n_groups, d_member_off, d_member_len,
                                      d_member_group, d_member_strand, n_members, band, max_err_pct, max_len, tmpl_counts, d_cons, d_cons_len,
                                      d_voters, d_member_out, d_votes, refused_group, stream_v, nullptr, nullptr);
}

int pc_consensus_round_quality(pc_ctx *c, const void *d_arena, const void *d_tmpl_arena, const int64_t *h_tmpl_off,
                               const int32_t *h_tmpl_len, const int64_t *h_group_first, int64_t n_groups, const int64_t *d_member_off,
                               const int32_t *d_member_len, const int32_t *d_member_group, const uint8_t *d_member_strand,
                               int64_t n_members, int band, int max_err_pct, int max_len, int tmpl_counts, uint8_t *d_cons,
                               int32_t *d_cons_len, int32_t *d_voters, int32_t *d_member_out, uint32_t *d_votes, int64_t *refused_group,
                               void *stream_v, const uint8_t *h_qtab, uint8_t *d_qual)
{
    if (refused_group) *refused_group = -1;
    if ((h_qtab == nullptr) != (d_qual == nullptr)) return PC_ERR_BAD_ARG;
    if (h_qtab)
        for (int m = 0; m < pcc::QUAL_ENTRIES; ++m)
            if (h_qtab[m] > pcc::MAX_QUAL) return PC_ERR_BAD_ARG;
    if (!c || n_groups < 0 || n_members < 0 || n_groups > (int64_t)INT32_MAX || n_members > (int64_t)INT32_MAX) return PC_ERR_BAD_ARG;
    if (band < 1 || band > pcc::MAX_BAND || max_len < 1 || max_len > pcc::MAX_LEN_LIMIT) return PC_ERR_BAD_ARG;
    if (max_err_pct < 0 || max_err_pct > 100 || tmpl_counts < 0 || tmpl_counts > 1) return PC_ERR_BAD_ARG;
    if (n_groups == 0 || n_members == 0) return PC_OK;
    if (!d_arena || !d_tmpl_arena || !h_tmpl_off || !h_tmpl_len || !h_group_first || !d_member_off || !d_member_len || !d_member_group ||
        !d_cons || !d_cons_len || !d_voters || !d_member_out)
        return PC_ERR_BAD_ARG;
    if (h_group_first[0] != 0 || h_group_first[n_groups] != n_members) return PC_ERR_BAD_ARG;
    for (int64_t g = 0; g < n_groups; ++g)
        if (h_tmpl_len[g] < 1 || h_tmpl_off[g] < 0 || h_group_first[g + 1] < h_group_first[g]) return PC_ERR_BAD_ARG;

    // the per-group tables: a template above max_len is the kernels' to report, and is sized as max_len here
    std::vector<int64_t> meta((size_t)n_groups * 3 + ((size_t)n_groups + 1) / 2);
    int64_t *vote_off = meta.data() + n_groups, *cons_off = meta.data() + 2 * n_groups;
    int32_t *tmpl_len = (int32_t *)(meta.data() + 3 * n_groups);
    int64_t votes_at = 0, cons_at = 0;
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t la = std::min(h_tmpl_len[g], max_len);
        meta[(size_t)g] = h_tmpl_off[g];
        vote_off[g] = votes_at; cons_off[g] = cons_at; tmpl_len[g] = h_tmpl_len[g];
        votes_at += pcc::votes_per_group(la);
        cons_at += pcc::cons_capacity(la);
    }
    // slices of whole groups whose votes and trace fit the budget; never fewer than one group
    size_t budget = kConsensusScratchMB << 20;
    if (const char *e = getenv("PC_CONSENSUS_SCRATCH_MB")) { if (atol(e) > 0) budget = (size_t)atol(e) << 20; }
    struct Slice { int64_t g0, g1, rows; size_t votes, trace; };
    std::vector<Slice> slices;
    for (int64_t g0 = 0; g0 < n_groups;) {
        Slice s{g0, g0, 0, 0, 0};
        while (s.g1 < n_groups) {
            const int64_t la = std::min(h_tmpl_len[s.g1], max_len);
            const int64_t rows = std::max(s.rows, la + 1), members = h_group_first[s.g1 + 1] - h_group_first[g0];
            const size_t votes = s.votes + (size_t)pcc::votes_per_group(la) * 4;
            const size_t trace = (size_t)members * (size_t)rows * pcc::TRACE_ROW_BYTES;
            if (votes + trace > budget) break;
            s.g1 += 1; s.rows = rows; s.votes = votes; s.trace = trace;
        }
        if (s.g1 == g0) {                                           // this group alone is above the budget
            if (refused_group) *refused_group = g0;
            return PC_ERR_OVER_BUDGET;
        }
        slices.push_back(s);
        g0 = s.g1;
    }
    size_t votes_max = 0, trace_max = 0;
    for (const Slice &s : slices) { votes_max = std::max(votes_max, s.votes); trace_max = std::max(trace_max, s.trace); }

    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipStreamSynchronize(stream));                           // the buffers below may still serve the call before this one
    int rc;
    if ((rc = c->d_cons_meta.ensure(meta.size() * 8))) return rc;
    if ((rc = c->d_cons_trace.ensure(trace_max + 256))) return rc;
    if (!d_votes && (rc = c->d_cons_votes.ensure(votes_max + 256))) return rc;
    HIP_TRY(hipMemcpy(c->d_cons_meta.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_voters, 0, (size_t)n_groups * 4, stream));

    pck::ConsensusArgs a{};
    a.arena = (const uint8_t *)d_arena; a.tmpl_arena = (const uint8_t *)d_tmpl_arena;
    a.tmpl_off = c->d_cons_meta.as<int64_t>(); a.vote_off = a.tmpl_off + n_groups; a.cons_off = a.tmpl_off + 2 * n_groups;
    a.tmpl_len = (const int32_t *)(a.tmpl_off + 3 * n_groups);
    a.member_off = d_member_off; a.member_len = d_member_len; a.member_group = d_member_group; a.member_strand = d_member_strand;
    a.n_groups_all = n_groups;
    a.trace = c->d_cons_trace.as<uint8_t>();
    a.band = band; a.max_err_pct = max_err_pct; a.max_len = max_len; a.tmpl_counts = tmpl_counts;
    a.member_out = d_member_out; a.voters = d_voters; a.cons = d_cons; a.cons_len = d_cons_len;
    a.err = c->d_err.as<uint32_t>();
    for (const Slice &s : slices) {
        a.first_group = s.g0; a.n_groups = s.g1 - s.g0;
        a.first_member = h_group_first[s.g0]; a.n_members = h_group_first[s.g1] - h_group_first[s.g0];
        a.rows = s.rows;
        if (d_votes) { a.votes = d_votes; a.vote_base = 0; }
        else { a.votes = c->d_cons_votes.as<uint32_t>(); a.vote_base = vote_off[s.g0]; }
        HIP_TRY(hipMemsetAsync(a.votes + (vote_off[s.g0] - a.vote_base), 0, s.votes, stream));
        if (pck::launch_consensus_pileup(a, stream)) return PC_ERR_NO_DEVICE;
        if (!d_qual) {                                              // the call as it was: the same kernel, the same bytes
            if (pck::launch_consensus_call(a, stream)) return PC_ERR_NO_DEVICE;
        } else {
            pck::ConsensusQualityArgs q;
            q.a = a;
            memcpy(q.qtab, h_qtab, sizeof q.qtab);
            q.qual = d_qual;
            if (pck::launch_consensus_call_quality(q, stream)) return PC_ERR_NO_DEVICE;
        }
    }
    return PC_OK;
}

int pc_path_cigar(const uint32_t *ops, int path_len, char *buf, size_t buflen)
{
    if (path_len < 0 || (path_len > 0 && !ops)) return 0;
    return pcpath::path_cigar(ops, path_len, buf, buflen);
}

int pc_trace_ops_x100(pc_ctx *c)
{
    if (!c) return 2100;
    // the end-window shape: the ligation adapters' row class, 150 columns
    return pcn::trace16_plan(plan_params(c), 28, 150) ? 1325 : 2100;
}

int pc_phase_b_reduce(pc_ctx *c, const int32_t *d_records, int64_t n, int njobs, const int64_t *job_record_offset,
                      const int32_t *job_side, int end_size, int min_trim_size, int extra_end_trim, double end_threshold,
                      int32_t *d_start_trim, int32_t *d_end_trim, int nbins, const int32_t *bin_start_job,
                      const int32_t *bin_end_job, double barcode_threshold, double barcode_diff, int require_two,
                      int32_t *d_call, void *stream_v)
{
    return pc_phase_b_reduce_masked(c, d_records, n, njobs, job_record_offset, job_side, end_size, min_trim_size, extra_end_trim,
                                    end_threshold, d_start_trim, d_end_trim, nbins, bin_start_job, bin_end_job, barcode_threshold,
                                    barcode_diff, require_two, d_call, nullptr, stream_v);
}

int pc_phase_b_reduce_masked(pc_ctx *c, const int32_t *d_records, int64_t n, int njobs, const int64_t *job_record_offset,
                             const int32_t *job_side, int end_size, int min_trim_size, int extra_end_trim, double end_threshold,
                             int32_t *d_start_trim, int32_t *d_end_trim, int nbins, const int32_t *bin_start_job,
                             const int32_t *bin_end_job, double barcode_threshold, double barcode_diff, int require_two,
                             int32_t *d_call, const uint64_t *d_traced_mask, void *stream_v)
{
    if (!c || n < 0 || njobs < 0 || nbins < 0) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_start_trim || !d_end_trim || (njobs > 0 && (!d_records || !job_record_offset || !job_side))) return PC_ERR_BAD_ARG;
    if (nbins > 0 && (!bin_start_job || !bin_end_job || !d_call)) return PC_ERR_BAD_ARG;
    for (int k = 0; k < nbins; ++k)
        if (bin_start_job[k] >= njobs || bin_end_job[k] >= njobs) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    // tables: [njobs] int64 record offsets, then job_side[njobs], bin_start[nbins], bin_end[nbins] as int32 -- staged
    // in pinned host memory and copied asynchronously; the slot's previous user (two calls ago) has long finished
    c->red_slot ^= 1;
    const int sl = c->red_slot;
    HIP_TRY(hipEventSynchronize(c->red_done[sl]));
    const size_t off_bytes = ((size_t)std::max(njobs, 1) * 8 + 15) / 16 * 16;
    const size_t tab_ints = (size_t)njobs + 2 * (size_t)nbins;
    const size_t total = off_bytes + (tab_ints + 4) * 4;
    if (c->h_red_cap[sl] < total) {
        if (c->h_red[sl]) { (void)hipHostFree(c->h_red[sl]); c->h_red[sl] = nullptr; c->h_red_cap[sl] = 0; }
        HIP_TRY(hipHostMalloc(&c->h_red[sl], total * 2, hipHostMallocDefault));
        c->h_red_cap[sl] = total * 2;
    }
    int rc = c->d_red_slot[sl].ensure(total);
    if (rc) return rc;
    char *h = (char *)c->h_red[sl];
    if (njobs > 0) memcpy(h, job_record_offset, (size_t)njobs * 8);
    int32_t *tab = (int32_t *)(h + off_bytes);
    if (njobs > 0) memcpy(tab, job_side, (size_t)njobs * 4);
    if (nbins > 0) {
        memcpy(tab + njobs, bin_start_job, (size_t)nbins * 4);
        memcpy(tab + njobs + nbins, bin_end_job, (size_t)nbins * 4);
    }
    HIP_TRY(hipMemcpyAsync(c->d_red_slot[sl].p, h, total, hipMemcpyHostToDevice, stream));
    pck::ReduceArgs a;
    memset(&a, 0, sizeof(a));
    a.records = d_records; a.n = n; a.njobs = njobs;
    a.job_off = c->d_red_slot[sl].as<int64_t>();
    a.job_side = (const int32_t *)((char *)c->d_red_slot[sl].p + off_bytes);
    a.end_size = end_size; a.min_trim_size = min_trim_size; a.extra_end_trim = extra_end_trim; a.end_threshold = end_threshold;
    a.start_trim = d_start_trim; a.end_trim = d_end_trim;
    a.nbins = nbins; a.bin_start = a.job_side + njobs; a.bin_end = a.bin_start + nbins;
    a.barcode_threshold = barcode_threshold; a.barcode_diff = barcode_diff; a.require_two = require_two ? 1 : 0;
    a.call = d_call;
    a.traced_mask = (const unsigned long long *)d_traced_mask; a.mask_words = (n + 63) / 64;
    if (pck::launch_reduce(a, stream)) return PC_ERR_NO_DEVICE;
    HIP_TRY(hipEventRecord(c->red_done[sl], stream));
    return PC_OK;
}

int pc_phase_b_explain(pc_ctx *c, const int32_t *d_records, int64_t n, int njobs, const int64_t *job_record_offset,
                       const int32_t *job_side, int end_size, int min_trim_size, int extra_end_trim, double end_threshold,
                       int nbins, const int32_t *bin_start_job, const int32_t *bin_end_job, const uint64_t *d_traced_mask,
                       int32_t *d_summary, double *d_bscore, const int64_t *d_hit_first, int32_t *d_hits, void *stream_v)
{
    static_assert(PC_EXPLAIN_INTS == pck::EXPLAIN_INTS, "the header and the kernel disagree on the summary layout");
    if (!c || n < 0 || njobs < 0 || nbins < 0) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    const bool fill = d_hit_first != nullptr;
    if (!d_summary || (!fill && !d_bscore) || (njobs > 0 && (!d_records || !job_record_offset || !job_side))) return PC_ERR_BAD_ARG;
    if (nbins > 0 && (!bin_start_job || !bin_end_job)) return PC_ERR_BAD_ARG;
    for (int k = 0; k < nbins; ++k)
        if (bin_start_job[k] >= njobs || bin_end_job[k] >= njobs) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    // tables, staged like pc_phase_b_reduce's (the same two slots): [njobs] int64 record offsets, then as int32
    // job_side[njobs], bin_start[nbins], bin_end[nbins], job_sbin[njobs], job_ebin[njobs]
    c->red_slot ^= 1;
    const int sl = c->red_slot;
    HIP_TRY(hipEventSynchronize(c->red_done[sl]));
    const size_t off_bytes = ((size_t)std::max(njobs, 1) * 8 + 15) / 16 * 16;
    const size_t tab_ints = 3 * (size_t)njobs + 2 * (size_t)nbins;
    const size_t total = off_bytes + (tab_ints + 4) * 4;
    if (c->h_red_cap[sl] < total) {
        if (c->h_red[sl]) { (void)hipHostFree(c->h_red[sl]); c->h_red[sl] = nullptr; c->h_red_cap[sl] = 0; }
        HIP_TRY(hipHostMalloc(&c->h_red[sl], total * 2, hipHostMallocDefault));
        c->h_red_cap[sl] = total * 2;
    }
    int rc = c->d_red_slot[sl].ensure(total);
    if (rc) return rc;
    char *h = (char *)c->h_red[sl];
    if (njobs > 0) memcpy(h, job_record_offset, (size_t)njobs * 8);
    int32_t *tab = (int32_t *)(h + off_bytes);
    if (njobs > 0) memcpy(tab, job_side, (size_t)njobs * 4);
    int32_t *h_bs = tab + njobs, *h_be = h_bs + nbins, *h_sbin = h_be + nbins, *h_ebin = h_sbin + njobs;
    // job -> bin, so that the kernel meets every barcode entry in its one walk over the jobs; a job that is the entry of
    // two bins on one side has no inverse (the kernel walks the bins instead)
    bool invertible = true;
    for (int j = 0; j < njobs; ++j) h_sbin[j] = h_ebin[j] = -1;
    for (int k = 0; k < nbins; ++k) {
        h_bs[k] = bin_start_job[k]; h_be[k] = bin_end_job[k];
        if (h_bs[k] >= 0) { if (h_sbin[h_bs[k]] >= 0) invertible = false; h_sbin[h_bs[k]] = k; }
        if (h_be[k] >= 0) { if (h_ebin[h_be[k]] >= 0) invertible = false; h_ebin[h_be[k]] = k; }
    }
    HIP_TRY(hipMemcpyAsync(c->d_red_slot[sl].p, h, total, hipMemcpyHostToDevice, stream));
    pck::ExplainArgs a;
    memset(&a, 0, sizeof(a));
    a.records = d_records; a.n = n; a.njobs = njobs;
    a.job_off = c->d_red_slot[sl].as<int64_t>();
    a.job_side = (const int32_t *)((char *)c->d_red_slot[sl].p + off_bytes);
    a.end_size = end_size; a.min_trim_size = min_trim_size; a.extra_end_trim = extra_end_trim; a.end_threshold = end_threshold;
    a.nbins = nbins; a.bin_start = a.job_side + njobs; a.bin_end = a.bin_start + nbins;
    if (invertible && nbins > 0) { a.job_sbin = a.bin_end + nbins; a.job_ebin = a.job_sbin + njobs; }
    a.traced_mask = (const unsigned long long *)d_traced_mask; a.mask_words = (n + 63) / 64;
    a.summary = d_summary; a.bscore = d_bscore; a.hit_first = d_hit_first; a.hits = d_hits;
    if (pck::launch_explain(a, stream)) return PC_ERR_NO_DEVICE;
    HIP_TRY(hipEventRecord(c->red_done[sl], stream));
    return PC_OK;
}

int pc_phase_b_select(pc_ctx *c, const int32_t *d_records, int64_t n, int njobs, const int64_t *d_job_record_offset,
                      const int32_t *d_job_side, const int32_t *d_job_adapter_len, const int32_t *d_job_calls,
                      const int32_t *d_start_len, const int32_t *d_end_len, int end_size, int min_trim_size,
                      int extra_end_trim, double end_threshold, int round, double call_level, double call_level_diff,
                      const uint64_t *d_mask_prev, const int32_t *d_start_trim, const int32_t *d_end_trim,
                      const double *d_best_full, uint64_t *d_mask_out, uint64_t *d_counts, int32_t *d_ub_trim_out,
                      double *d_ub_full_out, void *stream_v)
{
    if (!c || n < 0 || njobs < 0 || (round != 1 && round != 2)) return PC_ERR_BAD_ARG;
    if (n == 0 || njobs == 0) return PC_OK;
    if (!d_records || !d_job_record_offset || !d_job_side || !d_job_adapter_len || !d_job_calls || !d_start_len || !d_end_len ||
        !d_mask_out || !d_counts)
        return PC_ERR_BAD_ARG;
    if (round == 2 && (!d_mask_prev || !d_start_trim || !d_end_trim || (call_level < 1e8 && !d_best_full))) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    pck::SelectArgs a;
    memset(&a, 0, sizeof(a));
    a.records = d_records; a.n = n; a.njobs = njobs; a.job_off = d_job_record_offset;
    a.job_side = d_job_side; a.job_len = d_job_adapter_len; a.job_call = d_job_calls;
    a.start_len = d_start_len; a.end_len = d_end_len;
    a.end_size = end_size; a.min_trim_size = min_trim_size; a.extra_end_trim = extra_end_trim;
    a.match = c->match; a.gap_open = c->gap_open; a.gap_extend = c->gap_extend;
    a.pen_max = std::max(std::max(-c->mismatch, -c->gap_open), std::max(-c->gap_extend, 0));
    const double tau = (end_threshold - 1e-6) / 100.0;
    a.ident_c = tau * (double)c->match - (1.0 - tau) * (double)a.pen_max;
    a.round = round; a.call_level = call_level; a.call_level_diff = call_level_diff;
    a.mask_prev = (const unsigned long long *)d_mask_prev; a.start_trim = d_start_trim; a.end_trim = d_end_trim;
    a.best_full = d_best_full;
    a.mask_out = (unsigned long long *)d_mask_out; a.words = (n + 63) / 64; a.counts = (unsigned long long *)d_counts;
    a.ub_trim_out = round == 1 ? d_ub_trim_out : nullptr; a.ub_full_out = round == 1 ? d_ub_full_out : nullptr;
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)njobs * 8, stream));
    ScopedTimer tm(c, stream, 6, n * (int64_t)njobs);
    return pck::launch_select(a, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_phase_b_gather(pc_ctx *c, const uint64_t *d_mask, int64_t n, int njobs, const int64_t *d_job_first, uint64_t *d_cursor,
                      const int64_t *d_job_record_offset, const int32_t *d_job_side, const int64_t *d_start_off,
                      const int32_t *d_start_len, const int64_t *d_end_off, const int32_t *d_end_len, int64_t *d_win_off,
                      int32_t *d_win_len, int64_t *d_dest, int32_t *d_pair_job, int64_t *d_pair_read, void *stream_v)
{
    if (!c || n < 0 || njobs < 0) return PC_ERR_BAD_ARG;
    if (n == 0 || njobs == 0) return PC_OK;
    if (!d_mask || !d_job_first || !d_cursor || !d_job_record_offset || !d_job_side || !d_start_off || !d_start_len || !d_end_off ||
        !d_end_len || !d_win_off || !d_win_len || !d_dest || !d_pair_job || !d_pair_read || njobs > 65535)
        return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    pck::GatherArgs a;
    memset(&a, 0, sizeof(a));
    a.mask = (const unsigned long long *)d_mask; a.words = (n + 63) / 64; a.njobs = njobs;
    a.first = d_job_first; a.cursor = (unsigned long long *)d_cursor; a.job_off = d_job_record_offset; a.job_side = d_job_side;
    a.start_off = d_start_off; a.end_off = d_end_off; a.start_len = d_start_len; a.end_len = d_end_len;
    a.win_off = d_win_off; a.win_len = d_win_len; a.dest = d_dest; a.pair_job = d_pair_job; a.pair_read = d_pair_read;
    HIP_TRY(hipMemsetAsync(d_cursor, 0, (size_t)njobs * 8, stream));
    ScopedTimer tm(c, stream, 6, n * (int64_t)njobs);
    return pck::launch_gather(a, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_gather_records(pc_ctx *c, const int32_t *d_records, const int64_t *d_index, int64_t count, int32_t *d_out, void *stream_v)
{
    if (!c || count < 0) return PC_ERR_BAD_ARG;
    if (count == 0) return PC_OK;
    if (!d_records || !d_index || !d_out) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    ScopedTimer tm(c, stream, 6, count);
    return pck::launch_gather_records(d_records, d_index, count, d_out, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_phase_b_scatter(pc_ctx *c, const int32_t *d_traced, int64_t count, const int64_t *d_dest, const int32_t *d_pair_job,
                       const int64_t *d_pair_read, int32_t *d_records, const int32_t *d_job_side, const int32_t *d_job_calls,
                       double *d_best_full, int64_t n, void *stream_v)
{
    if (!c || count < 0 || n < 0) return PC_ERR_BAD_ARG;
    if (count == 0) return PC_OK;
    if (!d_traced || !d_dest || !d_pair_job || !d_pair_read || !d_records || !d_job_side || !d_job_calls) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    pck::ScatterArgs a;
    memset(&a, 0, sizeof(a));
    a.traced = d_traced; a.count = count; a.dest = d_dest; a.pair_job = d_pair_job; a.pair_read = d_pair_read;
    a.records = d_records; a.job_side = d_job_side; a.job_call = d_job_calls; a.best_full = d_best_full; a.n = n;
    ScopedTimer tm(c, stream, 6, count);
    return pck::launch_scatter(a, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_copy_windows(pc_ctx *c, const void *d_arena, const int64_t *d_src_off, const int32_t *d_len, int64_t n,
                    void *d_dst, const int64_t *d_dst_off, int pad, void *stream_v)
{
    if (!c || n < 0) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_arena || !d_src_off || !d_len || !d_dst || !d_dst_off || n > (int64_t)INT32_MAX) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    return pck::launch_copy_windows((const uint8_t *)d_arena, d_src_off, d_len, n, (uint8_t *)d_dst, d_dst_off, pad, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

// ---- the glue of the middle scan as single launches (pc_middle.hip); every pointer is device memory of the caller ---------------
int pc_trim_windows(pc_ctx *c, const int64_t *d_off, const int32_t *d_len, const int32_t *d_start_trim, const int32_t *d_end_trim, int64_t n,
                    int64_t *d_toff, int32_t *d_tlen, int64_t *d_stats, void *stream_v)
{
    if (!c || n < 0 || (n > 0 && (!d_off || !d_len || !d_start_trim || !d_end_trim || !d_toff || !d_tlen)) || !d_stats) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_stats, 0, 32, stream));      // (statistics that need another neutral element are stored offset: pc_middle.hip)
    return pck::launch_trim_windows(d_off, d_len, d_start_trim, d_end_trim, n, d_toff, d_tlen, d_stats, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_middle_hits(pc_ctx *c, const int32_t *d_records, int64_t n, double threshold, double *d_full, uint8_t *d_hit, void *stream_v)
{
    if (!c || n < 0 || (n > 0 && (!d_records || !d_full || !d_hit))) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    return pck::launch_middle_hits(d_records, n, threshold, d_full, d_hit, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

// ---- adapter discovery: the k-mer census and its candidate list (pc_discover.hip) ---------------------------------------------
int pc_kmer_count(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len, int64_t n, int k, uint32_t *d_counts,
                  void *stream_v)
{
    if (!c || k < 4 || k > 13 || n < 0) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_arena || !d_win_off || !d_win_len || !d_counts) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    return pck::launch_kmer_count((const uint8_t *)d_arena, d_win_off, d_win_len, n, k, d_counts, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_kmer_select(pc_ctx *c, const uint32_t *d_counts, int k, uint32_t min_count, int32_t *d_codes, uint32_t *d_cnt, int64_t cap,
                   int64_t *d_found, void *stream_v)
{
    if (!c || k < 4 || k > 13 || cap < 0 || !d_counts || !d_found || (cap > 0 && (!d_codes || !d_cnt))) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_found, 0, 8, stream));
    return pck::launch_kmer_select(d_counts, k, min_count, d_codes, d_cnt, cap, (unsigned long long *)d_found, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_anchor_inserts(pc_ctx *c, const uint8_t *d_arena, const int64_t *d_win_off, const int32_t *d_win_len, const int32_t *d_records,
                      int64_t n, int anchor_len, int side, int min_identity, int insert_len, int64_t *d_codes, void *stream_v)
{
    if (!c || n < 0 || anchor_len < 1 || side < 0 || side > 1 || min_identity < 0 || min_identity > 100 || insert_len < 1 || insert_len > 32)
        return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_arena || !d_win_off || !d_win_len || !d_records || !d_codes) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    return pck::launch_anchor_inserts(d_arena, d_win_off, d_win_len, d_records, n, anchor_len, side, min_identity, insert_len, d_codes, stream)
               ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_group_survivors(pc_ctx *c, const int32_t *d_mask, int64_t n, int words, const int32_t *d_gmask, int ngroups, uint8_t *d_cand,
                       int64_t *d_counts, void *stream_v)
{
    if (!c || n < 0 || words < 1 || ngroups < 0 || !d_counts || (n > 0 && ngroups > 0 && (!d_mask || !d_gmask || !d_cand))) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    if (ngroups > 0) HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)ngroups * 8, stream));
    return pck::launch_group_survivors(d_mask, n, words, d_gmask, ngroups, d_cand, d_counts, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_round_consume(pc_ctx *c, const double *d_full_all, const int32_t *d_rec_all, const int64_t *d_cur, const int64_t *d_act, int64_t nact,
                     int nadapters, int64_t ndirty, double threshold, uint8_t *d_anyh, int32_t *d_a_hit, int64_t *d_cnt, int64_t *d_stats,
                     void *stream_v)
{
    if (!c || nact < 0 || nadapters < 1 || ndirty < 0 || !d_stats) return PC_ERR_BAD_ARG;
    if (nact > 0 && (!d_full_all || !d_rec_all || !d_cur || !d_act || !d_anyh || !d_a_hit || !d_cnt)) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_stats, 0, 32, stream));
    return pck::launch_round_consume(d_full_all, d_rec_all, d_cur, d_act, nact, nadapters, ndirty, threshold, d_anyh, d_a_hit, d_cnt, d_stats, stream)
               ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_round_select(pc_ctx *c, const int32_t *d_rec_all, const int64_t *d_act, const uint8_t *d_anyh, const int32_t *d_a_hit,
                    const int32_t *d_set_of, int64_t nact, int nadapters, int64_t ndirty, int nsets, int floored_positive,
                    uint8_t *d_need, int64_t *d_counts, void *stream_v)
{
    if (!c || nact < 0 || nadapters < 1 || ndirty < 0 || nsets < 1 || !d_counts || !d_set_of) return PC_ERR_BAD_ARG;
    if (nact > 0 && (!d_rec_all || !d_act || !d_anyh || !d_a_hit || !d_need)) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nsets * 8, stream));
    if (nact > 0) HIP_TRY(hipMemsetAsync(d_need, 0, (size_t)nsets * (size_t)nact, stream));
    return pck::launch_round_select(d_rec_all, d_act, d_anyh, d_a_hit, d_set_of, nact, nadapters, ndirty, nsets, floored_positive, d_need,
                                    d_counts, stream)
               ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_mask_rule_gate(const char *const *adapters, int nadapters, int match, int mismatch, int gap_open, int gap_extend, int wildcards)
{
    if (nadapters < 0 || (nadapters > 0 && !adapters)) return 0;
    std::vector<int> lens;
    for (int i = 0; i < nadapters; ++i) {
        if (!adapters[i]) return 0;
        lens.push_back((int)strlen(adapters[i]));
    }
    return pcm::gate(adapters, lens.data(), nadapters, match, mismatch, gap_open, gap_extend, wildcards != 0) ? 1 : 0;
}

int pc_mask_rule_must_realign(int adapter, int cur, int32_t read_start, int32_t read_end, int32_t mask_start, int32_t mask_end,
                              int floored_positive)
{
    return pcm::must_realign(adapter, cur, read_start, read_end, mask_start, mask_end, floored_positive != 0) ? 1 : 0;
}

int pc_unpack_device(pc_ctx *c, const void *d_packed, int64_t nbases, const int64_t *d_exc_pos, int64_t nexc, void *d_arena,
                     int pad_bytes, void *stream_v)
{
    if (!c || nbases < 0 || nexc < 0 || pad_bytes < 0) return PC_ERR_BAD_ARG;
    if (nbases + pad_bytes == 0) return PC_OK;
    if (!d_arena || (nbases && !d_packed) || (nexc && !d_exc_pos)) return PC_ERR_BAD_ARG;
    if (((uintptr_t)d_packed & 3u) || ((uintptr_t)d_arena & 15u)) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    return pck::launch_unpack(d_packed, nbases, d_exc_pos, nexc, d_arena, pad_bytes, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_prefilter_max_edits(int adapter_len, double threshold_percent) { return pcp::max_edits(adapter_len, threshold_percent); }

// ---- the exact prefilter: one plan (pc_prefilter_plan.h) cached on the device, and the launches over it -------------------------
namespace {

static_assert(pcp::kBitmapWords == pck::kSeedBitmapWords, "the plan lays the seed bitmaps out as the scan kernels read them");

int upload_plan(pc_ctx *c, const pcp::Plan &p, hipStream_t stream)
{
    int rc;
    if (p.nq > 0) {
        HIP_TRY(hipStreamSynchronize(stream));
        if ((rc = c->d_sd_bitmaps.ensure(p.bitmaps.size() * 4)) || (rc = c->d_sd_first.ensure(p.first.size() * 4)) ||
            (rc = c->d_sd_entries.ensure(p.entries.size() * 4)) || (rc = c->d_sd_meta.ensure(p.piece_meta.size() * 4)) ||
            (rc = c->d_sd_eq.ensure(p.piece_eq.size() * 4)) || (rc = c->d_sd_count.ensure(64)))
            return rc;
        HIP_TRY(hipMemcpy(c->d_sd_bitmaps.p, p.bitmaps.data(), p.bitmaps.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_sd_first.p, p.first.data(), p.first.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_sd_entries.p, p.entries.data(), p.entries.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_sd_meta.p, p.piece_meta.data(), p.piece_meta.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_sd_eq.p, p.piece_eq.data(), p.piece_eq.size() * 4, hipMemcpyHostToDevice));
        if (!c->h_sd_count) HIP_TRY(hipHostMalloc((void **)&c->h_sd_count, 64, hipHostMallocDefault));
    }
    // the tables of the previous list may still be read by a launch in flight on the caller's stream
    HIP_TRY(hipStreamSynchronize(stream));
    if ((rc = c->d_pf_tables.ensure(p.tables.size() * 4)) || (rc = c->d_pf_meta.ensure(p.meta.size() * 4))) return rc;
    HIP_TRY(hipMemcpy(c->d_pf_tables.p, p.tables.data(), p.tables.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_pf_meta.p, p.meta.data(), p.meta.size() * 4, hipMemcpyHostToDevice));
    return PC_OK;
}

int prefilter_impl(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                   int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits, int nadapters,
                   uint32_t *d_mask, void *stream_v, pcp::Route route)
{
    if (!c || nwindows < 0 || nadapters < 0 || max_len < 0) return PC_ERR_BAD_ARG;
    if (nwindows == 0 || nadapters == 0) return PC_OK;
    if (!d_arena || !d_win_off || !d_win_len || !adapters || !max_edits || !d_mask) return PC_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    const int words = (nadapters + 31) / 32;
    const bool plane = route != pcp::Route::Bytes;
    std::vector<int32_t> key(adapters, adapters + nadapters);
    key.insert(key.end(), max_edits, max_edits + nadapters);
    key.push_back((int32_t)route);
    key.push_back(c->wildcards ? 1 : 0);
    if (key != c->pf.key) {
        // PC_PF_NO_SEEDS=1: exhaustive kernel only; PC_PF_MULTI_Q=1 / PC_PF_SINGLE_Q=1 force the seed-length choice (read once per process)
        static const pcp::Options options = [] {
            auto on = [](const char *name) { const char *e = getenv(name); return e && *e && *e != '0'; };
            pcp::Options o;
            o.no_seeds = on("PC_PF_NO_SEEDS"); o.force_multi_q = on("PC_PF_MULTI_Q"); o.force_single_q = on("PC_PF_SINGLE_Q");
            return o;
        }();
        pcp::Plan fresh;
        if (pcp::build(c->adapters, adapters, max_edits, nadapters, route, options, fresh, c->wildcards)) return PC_ERR_BAD_ARG;
        if (route == pcp::Route::PlaneSeeds && !fresh.launches.empty() && !fresh.seeds_only) return PC_ERR_UNSUPPORTED_SCORES;
        c->pf.key.clear();                    // from here on the device's tables are no longer the cached plan's
        const int rc = upload_plan(c, fresh, stream);
        if (rc) return rc;
        c->pf.plan = std::move(fresh);
        c->pf.key = std::move(key);
    }
    const pcp::Plan &plan = c->pf.plan;
    HIP_TRY(hipMemsetAsync(d_mask, 0, (size_t)nwindows * words * 4, stream));
    if (plan.launches.empty() || max_len == 0) return PC_OK;
    if (route == pcp::Route::PlaneSeeds && !plan.seeds_only) return PC_ERR_UNSUPPORTED_SCORES;    // this route has the seed stage only
    // column chunks: enough (window, chunk) units to fill the chip several times over, chunks no shorter than 512
    // columns (the warm-up before a chunk is the longest piece + its edit bound: ~35 columns)
    const int64_t target = (int64_t)c->ncu * 2048 * 6;
    int64_t chunks = (target + nwindows - 1) / nwindows;
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, (max_len + 511) / 512));
    if (c->len_hint > 0 && (int64_t)c->len_hint * 2 < max_len)           // ragged lengths: chunks about as long as a typical read
        chunks = std::max<int64_t>(chunks, (max_len + c->len_hint - 1) / c->len_hint);
    int chunk_len = (int)(((int64_t)max_len + chunks - 1) / chunks);
    chunk_len = (chunk_len + 15) / 16 * 16;
    chunks = ((int64_t)max_len + chunk_len - 1) / chunk_len;
    pck::PrefilterArgs a;
    memset(&a, 0, sizeof a);
    a.arena = (const uint8_t *)d_arena; a.win_off = d_win_off; a.win_len = d_win_len; a.nwindows = nwindows;
    a.chunks = (int32_t)chunks; a.chunk_len = chunk_len; a.warm = plan.warm;
    a.mask = d_mask; a.words = words;
    a.max_len = max_len; a.err = c->d_err.as<uint32_t>();
    auto exhaustive = [&](const std::vector<pcp::Launch> &ls) -> int {
        for (const pcp::Launch &L : ls) {
            a.tables = c->d_pf_tables.as<uint32_t>() + L.table_off; a.piece_meta = c->d_pf_meta.as<int32_t>() + L.meta_off;
            if (route == pcp::Route::PlaneTotal ? pck::launch_prefilter_packed(a, L.P, L.groups, stream) : pck::launch_prefilter(a, L.P, L.groups, stream))
                return PC_ERR_NO_DEVICE;
        }
        return PC_OK;
    };
    ScopedTimer tm(c, stream, 4, nwindows * nadapters);              // the launches of one call are timed as ONE region
    if (plan.nq == 0) return exhaustive(plan.launches);
    // ---- seed stage: one pass over the reads finds the exact seeds, the finds are verified; the pieces without
    // seeds run the exhaustive kernel.  The candidate list is sized from the seeds' expected rate on random sequence
    // (x2 + slack, at most a sixteenth of the columns); a batch that overflows it -- low-complexity reads against a
    // low-complexity seed -- is redone by the exhaustive kernel: never much slower than that, never inexact.
    const double columns = (double)nwindows * ((c->len_hint > 0 && c->len_hint < max_len) ? (double)c->len_hint : (double)max_len);
    static const int64_t cap_env = [] { const char *e = getenv("PC_PF_SEED_CAP"); return e ? (int64_t)atoll(e) : (int64_t)0; }();
    int64_t cap = (int64_t)std::min(columns * plan.rate * 2.0 + 1e6, std::max(4e6, columns / 16.0));
    if (cap_env > 0) cap = cap_env;
    int rc = c->d_sd_cand.ensure((size_t)cap * 8 + 64);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_sd_count.p, 0, 8, stream));
    pck::SeedScanArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.arena = a.arena; sa.win_off = d_win_off; sa.win_len = d_win_len; sa.nwindows = nwindows;
    sa.chunks = a.chunks; sa.chunk_len = a.chunk_len; sa.warm = plan.q[0] - 1;
    sa.nq = plan.nq;
    for (int t = 0; t < 3; ++t) sa.q[t] = plan.q[t];
    sa.bitmaps = c->d_sd_bitmaps.as<uint32_t>();
    sa.cand = c->d_sd_cand.as<uint32_t>(); sa.count = c->d_sd_count.as<unsigned long long>(); sa.cap = cap;
    sa.max_len = max_len; sa.err = c->d_err.as<uint32_t>();
    {
        ScopedTimer ts(c, stream, 5, nwindows);     // the scan alone (pairs = windows)
        if (plane ? pck::launch_seed_scan_packed(sa, stream) : pck::launch_seed_scan(sa, stream)) return PC_ERR_NO_DEVICE;
    }
    if (route != pcp::Route::PlaneSeeds && (rc = exhaustive(plan.rest_launches))) return rc;     // independent of the candidate count
    auto verify = [&](int64_t ncand) -> int {
        pck::SeedVerifyArgs va;
        memset(&va, 0, sizeof va);
        va.arena = a.arena; va.win_off = d_win_off; va.win_len = d_win_len;
        va.cand = c->d_sd_cand.as<uint32_t>(); va.count = c->d_sd_count.as<unsigned long long>(); va.cap = cap;
        for (int t = 0; t < 3; ++t) { va.q[t] = plan.q[t]; va.first_off[t] = plan.first_off[t]; }
        va.first = c->d_sd_first.as<uint32_t>(); va.entries = c->d_sd_entries.as<int32_t>();
        va.piece_meta = c->d_sd_meta.as<int32_t>(); va.piece_eq = c->d_sd_eq.as<uint32_t>(); va.npieces = plan.npieces;
        va.mask = d_mask; va.words = words;
        return (plane ? pck::launch_seed_verify_packed(va, ncand, stream) : pck::launch_seed_verify(va, ncand, stream)) ? PC_ERR_NO_DEVICE : PC_OK;
    };
    c->pf_deferred_cap = 0;
    if (c->pf_defer_count) {
        // No host round trip: the verify kernels read the count on the device (threads beyond it leave at once) and are
        // launched for the whole list; the count travels to pinned host memory behind them, and the caller -- who
        // synchronises anyway to size the DP over the survivors -- asks pc_prefilter_overflowed afterwards (an overflowed
        // list is the rare case: the caller then repeats the call with the count read here, below).
        if ((rc = verify(cap))) return rc;
        *c->h_sd_count = 0;
        HIP_TRY(hipMemcpyAsync(c->h_sd_count, c->d_sd_count.p, 8, hipMemcpyDeviceToHost, stream));
        c->pf_deferred_cap = cap;
        return PC_OK;
    }
    HIP_TRY(hipMemcpyAsync(c->h_sd_count, c->d_sd_count.p, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));                          // the one host round trip of the stage
    const unsigned long long found = *c->h_sd_count;
    if (found > (unsigned long long)cap) {
        static bool told = false;
        if (!told) fprintf(stderr, "porechop_amd: %llu seed candidates for a list of %lld: this batch is filtered by the exhaustive kernel\n",
                           found, (long long)cap);
        told = true;
        if (route == pcp::Route::PlaneSeeds) {
            // this route has no exhaustive kernel: nothing is excluded for this batch (every pair goes to the DP -- exact, only slower)
            HIP_TRY(hipMemsetAsync(d_mask, 0xFF, (size_t)nwindows * words * 4, stream));
            return PC_OK;
        }
        HIP_TRY(hipMemsetAsync(d_mask, 0, (size_t)nwindows * words * 4, stream));
        return exhaustive(plan.launches);
    }
    return verify((int64_t)found);
}

}  // namespace

int pc_prefilter_device(pc_ctx *c, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                        int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits, int nadapters,
                        uint32_t *d_mask, void *stream_v)
{
    return prefilter_impl(c, d_arena, d_win_off, d_win_len, nwindows, max_len, adapters, max_edits, nadapters, d_mask, stream_v, pcp::Route::Bytes);
}

// The same decision over reads held at 2 bits per base (pc_pack_reads' plane; d_win_off counts BASES; the plane must be
// 16-byte aligned and readable 64 bytes past its last base).  Only the seed stage exists for this form: every adapter must be
// made of A/C/G/T(U) and seedable (parts of >= 6 bases, <= 7 edits) -- else PC_ERR_UNSUPPORTED_SCORES, and the caller unpacks
// the reads and takes pc_prefilter_device.  Bases that were not A/C/G/T/U are seen as 'A': against such adapters that can only
// add survivors, never remove one, so a cleared bit is still a proof.
int pc_prefilter_packed(pc_ctx *c, const void *d_plane, const int64_t *d_win_off, const int32_t *d_win_len,
                        int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits, int nadapters,
                        uint32_t *d_mask, void *stream_v)
{
    if (((uintptr_t)d_plane & 15u) != 0) return PC_ERR_BAD_ARG;
    return prefilter_impl(c, d_plane, d_win_off, d_win_len, nwindows, max_len, adapters, max_edits, nadapters, d_mask, stream_v, pcp::Route::PlaneSeeds);
}

// pc_prefilter_packed for EVERY adapter list and bound: what the seed stage cannot take (and a batch whose candidate list
// overflowed) runs the exhaustive kernel over the plane, prefilter_packed_kernel; adapter letters that are not A/C/G/T/U are
// wildcards there (pc_prefilter.hip: a cleared bit is still a proof).  Never PC_ERR_UNSUPPORTED_SCORES.
int pc_prefilter_packed_any(pc_ctx *c, const void *d_plane, const int64_t *d_win_off, const int32_t *d_win_len,
                            int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits, int nadapters,
                            uint32_t *d_mask, void *stream_v)
{
    if (((uintptr_t)d_plane & 15u) != 0) return PC_ERR_BAD_ARG;
    return prefilter_impl(c, d_plane, d_win_off, d_win_len, nwindows, max_len, adapters, max_edits, nadapters, d_mask, stream_v, pcp::Route::PlaneTotal);
}

int pc_unpack_windows(pc_ctx *c, const void *d_plane, const int64_t *d_exc_pos, int64_t nexc, const int64_t *d_src_off,
                      const int32_t *d_len, int64_t n, void *d_dst, const int64_t *d_dst_off, int pad, void *stream_v)
{
    if (!c || n < 0 || nexc < 0) return PC_ERR_BAD_ARG;
    if (n == 0) return PC_OK;
    if (!d_plane || !d_src_off || !d_len || !d_dst || !d_dst_off || (nexc && !d_exc_pos) || ((uintptr_t)d_plane & 3u)) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    return pck::launch_unpack_windows(d_plane, d_exc_pos, nexc, d_src_off, d_len, n, (uint8_t *)d_dst, d_dst_off, pad, stream) ? PC_ERR_NO_DEVICE : PC_OK;
}

int pc_prefilter_defer_count(pc_ctx *c, int enabled)
{
    if (!c) return PC_ERR_BAD_ARG;
    c->pf_defer_count = enabled != 0;
    return PC_OK;
}

int pc_prefilter_overflowed(pc_ctx *c)
{
    if (!c) return 0;
    return (c->pf_deferred_cap > 0 && c->h_sd_count && *c->h_sd_count > (unsigned long long)c->pf_deferred_cap) ? 1 : 0;
}

void pc_jit_async(int enabled) { pcj::set_async(enabled); }
void pc_jit_shutdown(void) { pcj::wait_idle(true); }

int pc_jit_precompile(const char *adapter_a, const char *adapter_b, int match, int mismatch, int gap_open, int gap_extend,
                      const char *cache_dir)
{
    if (!adapter_a || !*adapter_a) return PC_ERR_BAD_ARG;
    const std::string a = adapter_a, b = (adapter_b && *adapter_b) ? adapter_b : adapter_a;
    return pcj::precompile(a, b, match, mismatch, gap_open, gap_extend, cache_dir ? cache_dir : "");
}

int pc_jit_precompile_row_skip(const char *adapter_a, const char *adapter_b, int match, int mismatch, int gap_open, int gap_extend,
                               const char *cache_dir)
{
    if (!adapter_a || !*adapter_a) return PC_ERR_BAD_ARG;
    const std::string a = adapter_a, b = (adapter_b && *adapter_b) ? adapter_b : adapter_a;
    return pcj::precompile(a, b, match, mismatch, gap_open, gap_extend, cache_dir ? cache_dir : "", true);
}

void pc_jit_stats(int64_t *compiled, int64_t *from_disk)
{
    long c = 0, d = 0;
    pcj::stats(&c, &d);
    if (compiled) *compiled = c;
    if (from_disk) *from_disk = d;
}

int pc_set_timing(pc_ctx *c, int enabled)
{
    if (!c) return PC_ERR_BAD_ARG;
    c->timing = enabled != 0;
    return PC_OK;
}

int pc_get_timing(pc_ctx *c, void *stream_v, double *ms, int64_t *launches, int64_t *pairs)
{
    if (!c || !ms || !launches || !pairs) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < PC_KERNEL_KINDS; ++k) { ms[k] = 0.0; launches[k] = 0; pairs[k] = 0; }
    for (auto &t : c->timed) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, t.e0, t.e1) == hipSuccess) { ms[t.kind] += f; launches[t.kind] += 1; pairs[t.kind] += t.pairs; }
        (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1);
    }
    c->timed.clear();
    return PC_OK;
}

int pc_sync(pc_ctx *c, void *stream_v)
{
    if (!c) return PC_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    hipStream_t stream = (stream_v == PC_STREAM_CONTEXT) ? c->stream : (hipStream_t)stream_v;
    HIP_TRY(hipStreamSynchronize(stream));
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, c->d_err.p, 4, hipMemcpyDeviceToHost));
    if (err) {
        (void)hipMemset(c->d_err.p, 0, 4);
        fprintf(stderr, "porechop_amd: %u alignment(s) reported an internal inconsistency\n", err);
        return PC_ERR_INTERNAL;
    }
    return PC_OK;
}

int pc_align_batch_host(pc_ctx *c, const char *read_arena, int64_t arena_bytes, const int64_t *win_off,
                        const int32_t *win_len, const int32_t *adapter_idx, int64_t npairs, int mode, int32_t *out)
{
    if (!c || npairs < 0 || arena_bytes < 0) return PC_ERR_BAD_ARG;
    if (npairs == 0) return PC_OK;
    if (!read_arena || !win_off || !win_len || !adapter_idx || !out) return PC_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    (void)hipSetDevice(c->device);
    int rc = upload_panel(c);
    if (rc) return rc;
    const int nad = (int)c->adapters.size();

    // The read bytes start crossing PCIe FIRST (one asynchronous copy on the context's stream -- a direct DMA
    // when the caller's arena is pinned): validating, grouping and sorting the pairs below runs on the host
    // meanwhile, and nothing waits for the copy but the kernels, by stream order.
    if ((rc = c->d_arena.ensure((size_t)arena_bytes + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_arena.p, read_arena, (size_t)arena_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync((char *)c->d_arena.p + arena_bytes, 'N', 64, c->stream));
    auto drained = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };   // nothing in flight on a return

    // empties are answered here exactly as the reference reports them (alignment.cpp:9-21):
    // only field 0 (-1) and the score (INT_MIN, dp_algorithm_impl.h:1540-1541) are defined
    struct Key { int ad; int cls; int len; int64_t idx; };
    std::vector<Key> keys;
    keys.reserve((size_t)npairs);
    for (int64_t p = 0; p < npairs; ++p) {
        const int ad = adapter_idx[p];
        if (ad < 0 || ad >= nad || win_len[p] < 0 || win_off[p] < 0 || win_off[p] + win_len[p] > arena_bytes) return drained(PC_ERR_BAD_ARG);
        int32_t *o = out + p * PC_RESULT_INTS;
        if (win_len[p] == 0 || c->ad_len[ad] == 0) {
            o[0] = -1; o[1] = 0; o[2] = -1; o[3] = 0; o[4] = INT_MIN; o[5] = 0; o[6] = 0; o[7] = 0;
            continue;
        }
        const int window = c->ad_window[ad];
        const bool two = (mode == PC_MODE_TWO_PASS) || (mode == PC_MODE_AUTO && win_len[p] > 2 * window + 64);
        keys.push_back({ad, two ? 1 : 0, win_len[p], p});
    }
    if (keys.empty()) return drained(PC_OK);
    // group by (class, adapter); inside a job longest windows first so tiles are length-balanced
    std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
        if (a.cls != b.cls) return a.cls < b.cls;
        if (a.ad != b.ad) return a.ad < b.ad;
        if (a.len != b.len) return a.len > b.len;
        return a.idx < b.idx;
    });
    const size_t n = keys.size();
    std::vector<int64_t> s_off(n);
    std::vector<int32_t> s_len(n);
    for (size_t i = 0; i < n; ++i) { s_off[i] = win_off[keys[i].idx]; s_len[i] = keys[i].len; }

    if ((rc = c->d_woff.ensure(n * 8)) || (rc = c->d_wlen.ensure(n * 4)) || (rc = c->d_out.ensure(n * PC_RESULT_INTS * 4)))
        return drained(rc);
    // (s_off / s_len are locals: every return below goes through a stream synchronisation)
    if (hipMemcpyAsync(c->d_woff.p, s_off.data(), n * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->d_wlen.p, s_len.data(), n * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return drained(PC_ERR_NO_DEVICE);

    // one pc_scan_device call per class (their max_len differ by orders of magnitude)
    size_t i0 = 0;
    while (i0 < n) {
        size_t i1 = i0;
        while (i1 < n && keys[i1].cls == keys[i0].cls) ++i1;
        std::vector<int32_t> job_ad;
        std::vector<int64_t> job_start;
        int max_len = 0;
        for (size_t i = i0; i < i1; ++i) {
            if (i == i0 || keys[i].ad != keys[i - 1].ad) { job_ad.push_back(keys[i].ad); job_start.push_back((int64_t)(i - i0)); }
            max_len = std::max(max_len, keys[i].len);
        }
        job_start.push_back((int64_t)(i1 - i0));
        rc = pc_scan_device(c, c->d_arena.p, c->d_woff.as<int64_t>() + i0, c->d_wlen.as<int32_t>() + i0,
                            (int64_t)(i1 - i0), job_ad.data(), nullptr, job_start.data(), (int)job_ad.size(), max_len,
                            keys[i0].cls ? PC_MODE_TWO_PASS : PC_MODE_TRACE,
                            c->d_out.as<int32_t>() + i0 * PC_RESULT_INTS, c->stream);
        if (rc) return drained(rc);
        // the tile cache is keyed by the job table; descriptors differ per class, so drain here
        if ((rc = pc_sync(c, c->stream))) return drained(rc);
        i0 = i1;
    }
    std::vector<int32_t> tmp(n * PC_RESULT_INTS);
    HIP_TRY(hipMemcpy(tmp.data(), c->d_out.p, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
        memcpy(out + keys[i].idx * PC_RESULT_INTS, tmp.data() + i * PC_RESULT_INTS, PC_RESULT_INTS * 4);
    return PC_OK;
}

int pc_format_result(const int32_t *r, char *buf, size_t buflen)
{
    if (!r || !buf) return PC_ERR_BAD_ARG;
    if (r[0] == -1 && r[4] == INT_MIN) {
        // the reference leaves fields 1,3,5,6 uninitialised here; Porechop only tests field 0
        return snprintf(buf, buflen, "-1,0,-1,0,%d,0.000000,0.000000", INT_MIN);
    }
    // (100.0 * count) / length in double, evaluated at run time like alignment.cpp:81-82,89-90,
    // so a zero-length overlap prints this platform's 0.0/0.0 ("-nan" on x86-64 glibc)
    volatile double m = (double)r[5], al = (double)r[6], fl = (double)r[7];
    const double pa = 100.0 * m / al;
    const double pf = 100.0 * m / fl;
    return snprintf(buf, buflen, "%d,%d,%d,%d,%d,%f,%f", r[0], r[1], r[2], r[3], r[4], pa, pf);
}

int pc_format_results(const int32_t *recs, int64_t n, char *buf, int64_t buflen, int64_t *used)
{
    if (n < 0 || (n && (!recs || !buf))) return PC_ERR_BAD_ARG;
    int64_t pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (buflen - pos < 161) return PC_ERR_BAD_ARG;
        pos += pc_format_result(recs + i * PC_RESULT_INTS, buf + pos, 160);
        buf[pos++] = '\n';
    }
    if (used) *used = pos;
    return PC_OK;
}

// ---------------------------------------------------------------------------------------------
// process-wide default context + prefetch memo behind the reference's per-call symbol
// ---------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

struct MemoKey {
    uint64_t h1, h2;
    bool operator==(const MemoKey &o) const { return h1 == o.h1 && h2 == o.h2; }
};
struct MemoHash { size_t operator()(const MemoKey &k) const { return (size_t)(k.h1 ^ (k.h2 * 0x9E3779B97F4A7C15ull)); } };
// A hit is only a hit if the entry's own record of what it was computed for agrees: both lengths and a
// third, independently seeded 64-bit digest of (read bytes, adapter bytes, scores).  A collision of the
// 128-bit map key alone therefore cannot hand back another pair's alignment: it is treated as a miss.
struct MemoVal { int32_t r[PC_RESULT_INTS]; uint32_t n, m; uint64_t check; };
struct FullKey { MemoKey key; uint32_t n, m; uint64_t check; };

inline uint64_t mix64(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }

FullKey make_key(const char *rd, size_t n, const char *ad, size_t m, int a, int b, int o, int e)
{
    // three independent 64-bit hashes over (len, read bytes, adapter bytes, scores)
    uint64_t h1 = 0xcbf29ce484222325ull ^ n, h2 = 0x9ae16a3b2f90404full + m, h3 = 0x2545F4914F6CDD1Dull ^ (n * 0x9E3779B97F4A7C15ull) ^ m;
    auto feed = [&](const unsigned char *p, size_t len) {
        size_t i = 0;
        for (; i + 8 <= len; i += 8) {
            uint64_t w; memcpy(&w, p + i, 8);
            h1 = (h1 ^ w) * 0x100000001b3ull; h1 ^= h1 >> 29;
            h2 = mix64(h2 + w * 0x9E3779B97F4A7C15ull);
            h3 = (h3 ^ (w * 0xD6E8FEB86659FD93ull)) * 0xA0761D6478BD642Full; h3 ^= h3 >> 32;
        }
        uint64_t w = 0; memcpy(&w, p + i, len - i);
        w |= (uint64_t)(len - i) << 56;
        h1 = (h1 ^ w) * 0x100000001b3ull; h1 ^= h1 >> 29;
        h2 = mix64(h2 + w * 0x9E3779B97F4A7C15ull);
        h3 = (h3 ^ (w * 0xD6E8FEB86659FD93ull)) * 0xA0761D6478BD642Full; h3 ^= h3 >> 32;
    };
    feed((const unsigned char *)rd, n);
    feed((const unsigned char *)ad, m);
    // the four scores in full (int32 each), not truncated
    const uint64_t s1 = ((uint64_t)(uint32_t)a << 32) | (uint32_t)b, s2 = ((uint64_t)(uint32_t)o << 32) | (uint32_t)e;
    h1 = mix64(mix64(h1 ^ s1) + s2); h2 = mix64(mix64(h2 + s1) ^ s2); h3 = mix64(mix64(h3 ^ s2) + s1);
    return {{h1, h2}, (uint32_t)n, (uint32_t)m, h3};
}

struct Global {
    std::mutex mu;        // the memo and the adapter interning tables
    std::mutex gpu_mu;    // the default context (scores, panel, launches); always taken BEFORE mu, never after
    pc_ctx *ctx = nullptr;
    std::unordered_map<std::string, int> ad_index;
    std::vector<std::string> ad_list;
    std::unordered_map<MemoKey, MemoVal, MemoHash> memo;
    int64_t hits = 0, misses = 0, rejected = 0;
    size_t max_entries = 0;
};
Global &G()
{
    static Global g;
    static std::once_flag once;
    std::call_once(once, [] {
        // bounded: ~100 B per entry; when the bound is reached the memo starts over (an epoch clear --
        // Porechop's phases query each (window, adapter) pair at most a few times, close together)
        const char *e = getenv("PC_MEMO_MAX_ENTRIES");
        g.max_entries = e ? (size_t)atoll(e) : (size_t)4 << 20;
    });
    return g;
}

bool memo_lookup(Global &g, const FullKey &k, int32_t *rec)      // with g.mu held
{
    auto it = g.memo.find(k.key);
    if (it == g.memo.end()) return false;
    if (it->second.n != k.n || it->second.m != k.m || it->second.check != k.check) { ++g.rejected; return false; }
    memcpy(rec, it->second.r, sizeof(it->second.r));
    return true;
}

void memo_insert(Global &g, const FullKey &k, const int32_t *rec)   // with g.mu held
{
    if (g.max_entries && g.memo.size() >= g.max_entries) g.memo.clear();
    MemoVal v; memcpy(v.r, rec, sizeof(v.r)); v.n = k.n; v.m = k.m; v.check = k.check;
    g.memo[k.key] = v;
}

// with g.gpu_mu held
int default_ctx(int a, int b, int o, int e, pc_ctx **out)
{
    Global &g = G();
    if (!g.ctx) { int rc = pc_create(&g.ctx, -1); if (rc) return rc; }
    int rc = pc_set_scores(g.ctx, a, b, o, e);
    if (rc) return rc;
    *out = g.ctx;
    return PC_OK;
}

// with g.gpu_mu held
int intern_adapters(const char *const *seqs, int n, std::vector<int> &idx)
{
    Global &g = G();
    bool grew = false;
    idx.resize(n);
    {
        std::lock_guard<std::mutex> lk(g.mu);
        for (int i = 0; i < n; ++i) {
            std::string s(seqs[i]);
            if (s.size() > (size_t)PC_MAX_ADAPTER_ANY) return PC_ERR_ADAPTER_TOO_LONG;
            auto it = g.ad_index.find(s);
            if (it == g.ad_index.end()) { it = g.ad_index.emplace(s, (int)g.ad_list.size()).first; g.ad_list.push_back(s); grew = true; }
            idx[i] = it->second;
        }
    }
    if (grew || g.ctx->adapters.size() != g.ad_list.size()) {
        std::vector<const char *> ptrs;
        for (auto &s : g.ad_list) ptrs.push_back(s.c_str());
        return pc_set_adapters(g.ctx, ptrs.data(), (int)ptrs.size());
    }
    return PC_OK;
}

}  // namespace

extern "C" {

int pc_prefetch(const char *read_arena, int64_t arena_bytes, const int64_t *win_off, const int32_t *win_len,
                const char *const *adapters, const int32_t *adapter_idx, int64_t npairs, int match, int mismatch,
                int gap_open, int gap_extend)
{
    if (npairs <= 0) return PC_OK;
    if (!read_arena || !win_off || !win_len || !adapters || !adapter_idx) return PC_ERR_BAD_ARG;
    Global &g = G();
    std::lock_guard<std::mutex> gpu(g.gpu_mu);
    pc_ctx *c;
    int rc = default_ctx(match, mismatch, gap_open, gap_extend, &c);
    if (rc) return rc;
    int nad = 0;
    for (int64_t p = 0; p < npairs; ++p) nad = std::max(nad, adapter_idx[p] + 1);
    std::vector<int> gidx;
    if ((rc = intern_adapters(adapters, nad, gidx))) return rc;
    // skip what is already known
    std::vector<int64_t> todo;
    std::vector<FullKey> keys((size_t)npairs);
    std::vector<size_t> ad_len((size_t)nad);
    for (int i = 0; i < nad; ++i) ad_len[i] = strlen(adapters[i]);
    for (int64_t p = 0; p < npairs; ++p) {
        const char *ad = adapters[adapter_idx[p]];
        keys[p] = make_key(read_arena + win_off[p], (size_t)win_len[p], ad, ad_len[adapter_idx[p]], match, mismatch, gap_open, gap_extend);
    }
    {
        std::lock_guard<std::mutex> lk(g.mu);
        int32_t tmp[PC_RESULT_INTS];
        for (int64_t p = 0; p < npairs; ++p)
            if (!memo_lookup(g, keys[p], tmp)) todo.push_back(p);
    }
    if (todo.empty()) return PC_OK;
    std::vector<int64_t> off(todo.size());
    std::vector<int32_t> len(todo.size()), aidx(todo.size());
    for (size_t i = 0; i < todo.size(); ++i) { off[i] = win_off[todo[i]]; len[i] = win_len[todo[i]]; aidx[i] = gidx[adapter_idx[todo[i]]]; }
    std::vector<int32_t> res(todo.size() * PC_RESULT_INTS);
    rc = pc_align_batch_host(c, read_arena, arena_bytes, off.data(), len.data(), aidx.data(), (int64_t)todo.size(), PC_MODE_AUTO, res.data());
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g.mu);
    for (size_t i = 0; i < todo.size(); ++i) memo_insert(g, keys[todo[i]], res.data() + i * PC_RESULT_INTS);
    return PC_OK;
}

void pc_memo_clear(void)
{
    Global &g = G();
    std::lock_guard<std::mutex> lk(g.mu);
    g.memo.clear(); g.hits = g.misses = g.rejected = 0;
}

void pc_memo_stats(int64_t *hits, int64_t *misses, int64_t *entries)
{
    Global &g = G();
    std::lock_guard<std::mutex> lk(g.mu);
    if (hits) *hits = g.hits;
    if (misses) *misses = g.misses;
    if (entries) *entries = (int64_t)g.memo.size();
}

char *adapterAlignment(char *readSeq, char *adapterSeq, int matchScore, int mismatchScore, int gapOpenScore,
                       int gapExtensionScore)
{
    if (!readSeq || !adapterSeq) return nullptr;
    const size_t n = strlen(readSeq), m = strlen(adapterSeq);
    int32_t rec[PC_RESULT_INTS];
    Global &g = G();
    const FullKey key = make_key(readSeq, n, adapterSeq, m, matchScore, mismatchScore, gapOpenScore, gapExtensionScore);
    bool hit;
    {
        // hits never wait for the GPU: Porechop calls this from --threads Python threads at once
        // (porechop.py:309-322) and only the memo lookup is under the shared lock
        std::lock_guard<std::mutex> lk(g.mu);
        hit = memo_lookup(g, key, rec);
        if (hit) ++g.hits; else ++g.misses;
    }
    if (!hit) {
        if (n == 0 || m == 0) {
            rec[0] = -1; rec[1] = 0; rec[2] = -1; rec[3] = 0; rec[4] = INT_MIN; rec[5] = rec[6] = rec[7] = 0;
        } else {
            // a single-pair launch; misses queue up behind one another on the context, not behind hits
            std::lock_guard<std::mutex> gpu(g.gpu_mu);
            pc_ctx *c;
            int rc = default_ctx(matchScore, mismatchScore, gapOpenScore, gapExtensionScore, &c);
            std::vector<int> gidx;
            const char *ads[1] = {adapterSeq};
            if (!rc) rc = intern_adapters(ads, 1, gidx);
            const int64_t off = 0; const int32_t len = (int32_t)n, aidx = rc ? 0 : gidx[0];
            // Porechop asks for one pair at a time, but never for one pair only: a read's end window meets every sequence
            // of the panel in turn (phase A: porechop.py:296-322, nanopore_read.py:149-164) and every matching set's in phase
            // B.  A miss on a short window is therefore answered by ONE launch over that window against every adapter this
            // process has asked about so far (same scheme; packed kernels only), and all of it goes into the memo: the next
            // couple of hundred calls are lookups.  This is what makes "swap cpp_functions.so and change nothing else"
            // (INTEGRATION.md mode A) faster than the CPU instead of ten times slower: a single-pair launch costs ~125 us
            // whatever its size.  Whole reads (phase C asks for two or three adapters per read) stay single launches.
            static const bool no_spec = [] { const char *e = getenv("PC_NO_SPECULATION"); return e && *e && *e != '0'; }();
            bool speculated = false;
            // (upload_panel first: slow_scheme / ad_slow describe the scheme and panel just set)
            if (!rc && !no_spec && n <= 1024 && g.ad_list.size() > 1 && g.ad_list.size() <= 1024 &&
                (rc = upload_panel(c)) == PC_OK && !c->slow_scheme && !c->ad_slow[(size_t)aidx]) {
                std::vector<int32_t> ai, ln;
                std::vector<int64_t> of;
                for (size_t k = 0; k < g.ad_list.size(); ++k)
                    if (!c->ad_slow[k] && !g.ad_list[k].empty()) { ai.push_back((int32_t)k); ln.push_back((int32_t)n); of.push_back(0); }
                std::vector<int32_t> recs(ai.size() * PC_RESULT_INTS);
                rc = pc_align_batch_host(c, readSeq, (int64_t)n, of.data(), ln.data(), ai.data(), (int64_t)ai.size(), PC_MODE_AUTO, recs.data());
                if (!rc) {
                    std::lock_guard<std::mutex> lk(g.mu);
                    for (size_t i = 0; i < ai.size(); ++i) {
                        const std::string &ad = g.ad_list[(size_t)ai[i]];
                        const FullKey k2 = make_key(readSeq, n, ad.data(), ad.size(), matchScore, mismatchScore, gapOpenScore, gapExtensionScore);
                        memo_insert(g, k2, recs.data() + i * PC_RESULT_INTS);
                        if (ai[i] == aidx) memcpy(rec, recs.data() + i * PC_RESULT_INTS, sizeof(rec));
                    }
                    speculated = true;
                } else {
                    // the speculative batch failed (e.g. no room for its scratch): that is no reason to fail the ONE pair
                    // that was asked for -- fall through to the single-pair launch
                    rc = PC_OK;
                }
            }
            if (!rc && !speculated) rc = pc_align_batch_host(c, readSeq, (int64_t)n, &off, &len, &aidx, 1, PC_MODE_AUTO, rec);
            if (rc) {
                // Only a missing / failing device, scores above 2^20 in magnitude or an adapter above PC_MAX_ADAPTER_ANY
                // bases end here.  The unchanged Python wrapper dereferences the NULL below
                // (cpp_function_wrappers.py:56-63), so say clearly why before it does.
                fprintf(stderr, "porechop_amd: adapterAlignment cannot be computed on the GPU: %s (scores %d,%d,%d,%d; read of %zu, adapter of "
                                "%zu bases; limits: |score| <= 2^20, adapters up to %d bases, a visible MI355X).  Returning NULL.\n",
                        pc_strerror(rc), matchScore, mismatchScore, gapOpenScore, gapExtensionScore, n, m, PC_MAX_ADAPTER_ANY);
                return nullptr;
            }
        }
        std::lock_guard<std::mutex> lk(g.mu);
        memo_insert(g, key, rec);
    }
    char *buf = (char *)malloc(160);
    if (!buf) return nullptr;
    pc_format_result(rec, buf, 160);
    return buf;
}

void freeCString(char *p) { free(p); }

}  // extern "C"
