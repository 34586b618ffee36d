/*
 * porechop_amd.h -- C ABI of the MI355X-native adapter-alignment core (libporechop_amd.so,
 * also installable as Porechop's porechop/cpp_functions.so).
 *
 * Plain pointers and sizes only; no torch / HIP types.  Every entry point runs on the GPU:
 * there is NO CPU fallback anywhere behind this header (a missing device is an error).
 *
 * Part 1 is the reference's own FFI surface, kept bit-for-bit so that the unchanged
 * porechop/cpp_function_wrappers.py binds it.  Part 2 is the batch surface the reference does
 * not have (its API is one pair per call); it is what makes a GPU worthwhile.
 */
#ifndef PORECHOP_AMD_H
#define PORECHOP_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Part 1 -- drop-in replacements for the reference exports
 * ------------------------------------------------------------------------------------------ */

/* Replaces  porechop/include/adapter_align.h:12-16 / porechop/src/adapter_align.cpp:11-31
 * (bound by porechop/cpp_function_wrappers.py:27-33 with restype c_void_p).
 * Inputs are borrowed NUL-terminated ASCII strings.  Returns a malloc()ed C string
 *   "readStart,readEnd,adapterStart,adapterEnd,rawScore,alignedRegion%id,fullAdapter%id"
 * formatted exactly like porechop/src/alignment.cpp:113-121 ("%d" ints, "%f" doubles;
 * "-1,..." when either sequence is empty).  Served from the prefetch memo (Part 2) when the
 * pair is in it; otherwise by a GPU launch -- which, for a window of up to 1024 bases, covers that
 * window against EVERY adapter this process has asked about so far and memoises all of it (Porechop
 * walks a read's end window through the whole panel, porechop.py:296-322: one launch, then lookups;
 * PC_NO_SPECULATION=1 makes every miss a single-pair launch).  Any four integer scores (up to 2^20 in magnitude) and
 * adapters up to PC_MAX_ADAPTER_ANY bases are computed, as the reference computes them.  Never throws; on a device
 * error (or beyond those limits) it prints to stderr and returns NULL. */
char *adapterAlignment(char *readSeq, char *adapterSeq, int matchScore, int mismatchScore,
                       int gapOpenScore, int gapExtensionScore);

/* Replaces porechop/src/adapter_align.cpp:34-36 (cpp_function_wrappers.py:38-39): free(). */
void freeCString(char *p);

/* ------------------------------------------------------------------------------------------
 * Part 2 -- batch API
 * ------------------------------------------------------------------------------------------ */

typedef struct pc_ctx pc_ctx;

enum {
    PC_OK = 0,
    PC_ERR_NO_DEVICE = -1,          /* no HIP device / HIP call failed */
    PC_ERR_UNSUPPORTED_SCORES = -2, /* a score above 2^20 in magnitude, or sums that leave the 32-bit range */
    PC_ERR_BAD_ARG = -3,
    PC_ERR_ADAPTER_TOO_LONG = -4,   /* adapter longer than PC_MAX_ADAPTER_ANY */
    PC_ERR_INTERNAL = -5,           /* a kernel reported an inconsistency (never expected) */
    PC_ERR_OVER_BUDGET = -6         /* pc_consensus_round: one group alone needs more scratch than the budget allows */
};

#define PC_MAX_ADAPTER 128        /* the packed 16-bit kernels' limit; longer adapters take the plain-int32 kernel ... */
#define PC_MAX_ADAPTER_ANY 4096   /* ... up to this many bases */
#define PC_RESULT_INTS 8   /* readStart, readEnd, adapterStart, adapterEnd, rawScore,
                              matches, alignedRegionLength, fullAdapterLength.
                              identities are (100.0*matches)/length in double, as the reference
                              computes them (alignment.cpp:81-82,89-90); matches is the same
                              count for both.  Empty read or adapter: {-1,0,-1,0,INT_MIN,0,0,0}. */

/* `stream` arguments are hipStream_t handles passed as void*: NULL is HIP's default (null)
 * stream -- what torch.cuda.current_stream().cuda_stream is unless the caller changed it --
 * and PC_STREAM_CONTEXT selects the context's own non-blocking stream. */
#define PC_STREAM_CONTEXT ((void *)(intptr_t)-1)

/* scan modes */
#define PC_MODE_AUTO 0      /* by window length */
#define PC_MODE_TRACE 1     /* one pass, full trace (end windows) */
#define PC_MODE_TWO_PASS 2  /* score-only pass + bounded traced window (whole reads) */
#define PC_MODE_SCORE 3     /* score-only pass alone: records are (-2, J, I, 0, score, 0, 0, 0) -- the
                             * reference's end cell (row I of the adapter, window column J) and raw
                             * score, no traceback (pc_scan_device only) */

#define PC_MODE_TRACE_AT 4  /* the traced alignment of pairs whose END CELL is already known: on entry d_out holds, for
                             * every pair, the PC_MODE_SCORE record of the same (window, adapter) pair; on return the
                             * traced record.  Only the columns the path can occupy are traced (the last W + 2 before
                             * the end cell, W the exact bound of csrc/pc_bounds.h), the columns before them run the
                             * bare recurrence, the columns after the end cell are not run at all -- the machinery of
                             * PC_MODE_TWO_PASS's second pass, for windows of any length (phase B's exact pruning traces
                             * its few selected end-window pairs this way).  The score the window reproduces must equal
                             * the record's, or the pair is flagged (pc_sync: PC_ERR_INTERNAL).  pc_scan_device only. */

const char *pc_version(void);
const char *pc_strerror(int code);

/* 1 if (match, mismatch, gap_open, gap_extend) with adapters of up to max_adapter_len bases runs the PACKED 16-bit
 * kernels (match > 0, match > mismatch, negative gap scores, magnitudes that fit the int16 / fp16 lanes, adapters up to
 * PC_MAX_ADAPTER; gap_open == gap_extend selects the reference's linear-gap recurrence,
 * seqan/align/global_alignment_unbanded.h:217-220).  0: such pairs run the PLAIN-INT32 kernel (csrc/pc_slow.hip: one
 * lane per pair, every cell's trace kept) -- the same answers as the reference for ANY four integers up to 2^20 in
 * magnitude and adapters up to PC_MAX_ADAPTER_ANY, as porechop/porechop.py:145,196-202 accepts them, only about a
 * hundred times slower per cell and without the batch pipeline's exact prunings (PC_MODE_SCORE is refused there).
 * Nothing is ever approximated, and nothing runs on the CPU. */
int pc_scores_supported(int match, int mismatch, int gap_open, int gap_extend, int max_adapter_len);

/* device < 0: current device.  The context owns its stream-ordered scratch buffers. */
int pc_create(pc_ctx **ctx, int device);
void pc_destroy(pc_ctx *ctx);

/* The scoring scheme of the calls that follow; may be called on a live context, between any two calls.  Nothing is
 * uploaded here: a changed scheme only marks the panel dirty, and the NEXT call that needs the panel re-derives all of it
 * under the new scheme -- the adapters' windows and spans, which adapters take the plain-int32 kernel -- uploads it, and
 * drops the cached tile table and prefilter plan (it waits for the device first: earlier calls may still read the old
 * tables).  Magnitudes above 2^20 are refused and leave the scheme as it was. */
int pc_set_scores(pc_ctx *ctx, int match, int mismatch, int gap_open, int gap_extend);

/* IUPAC wildcards in ADAPTERS, a property of the context; off by default, and with it off every byte this library returns
 * is what it was before the mode existed.  With it on an adapter letter stands for a set of bases (csrc/pc_letters.h, the
 * one copy of the rule): A C G T, U = T, R = AG, Y = CT, S = CG, W = AT, K = GT, M = AC, B = CGT, D = AGT, H = ACT,
 * V = ACG, N = ACGT, either case, any other byte the empty set.  Read bytes stay Dna5: a cell scores `match` iff the read
 * base is one of A/C/G/T(U) and lies in the adapter letter's set, `mismatch` otherwise -- a read's N, '-' or IUPAC letter
 * matches nothing, not even adapter N, so a stretch masked by mask-and-realign is never a hit.  Recurrence, tie rules,
 * scout, traceback, digest and the two identities are unchanged; in a path '=' is a match under this rule.
 *   * An adapter of A/C/G/T/U alone gives the same records in both modes.  Every kernel takes the rule from a table of the
 *     rows' sets uploaded with the panel: trace16_kernel's substitution table, scan_kernel's wildcard variants, the specialised
 *     score kernels' tables (letters told apart by set; the in-memory kernel cache is keyed by the mode, the generated options
 *     of adapters without degenerate letters are unchanged), the plain-int32 and path kernels.  All modes, floors and the end
 *     rule work as without wildcards.  Under a scheme with max(match - mismatch, match) > 2048 scan_kernel's wildcard variants
 *     are not exact and are not launched at all: the adapters with other letters take the plain-int32 kernel (said once on
 *     stderr; PC_MODE_SCORE is then refused for them), every other adapter of the context the kernels it takes without
 *     wildcards, which are exact for it.
 *   * The prefilter stays a proof: a row's Eq bit is set for every base of its set, a piece with a degenerate letter has
 *     no seeds, and pc_prefilter_packed answers PC_ERR_UNSUPPORTED_SCORES for a list it cannot seed completely, as ever.
 *   * Like pc_set_scores this only marks the panel dirty: the next call that needs the panel re-derives and uploads it and
 *     drops the cached tile table and prefilter plan.  May be toggled on a live context between any two calls.
 *   * The per-call adapterAlignment symbol below never uses wildcards.
 * pc_letter_set: the 5-bit set over read codes 0..4 (A, C, G, T/U, other) of an adapter byte in either mode -- off: the
 * byte's own Dna5 code alone (N == N); on: the table above, bit 4 never set.  0 for a byte outside 0..255. */
int pc_set_wildcards(pc_ctx *ctx, int enabled);
int pc_letter_set(int byte, int wildcards);

/* Upload the adapter panel (the strings of porechop/adapters.py ADAPTERS start/end sequences
 * or any other): adapter index i in the calls below refers to seqs[i]. */
int pc_set_adapters(pc_ctx *ctx, const char *const *seqs, int nadapters);

/* Host-buffer batch: pair p aligns window  read_arena[win_off[p] .. win_off[p]+win_len[p])
 * against adapter adapter_idx[p]; results out[p*PC_RESULT_INTS ...].  Pairs may come in any
 * order; the library groups them.  Blocking. */
int pc_align_batch_host(pc_ctx *ctx, const char *read_arena, int64_t arena_bytes,
                        const int64_t *win_off, const int32_t *win_len, const int32_t *adapter_idx,
                        int64_t npairs, int mode, int32_t *out);

/* Device-buffer batch (inputs already resident in HBM; nothing crosses PCIe but the small job
 * table).  d_* are device pointers.  d_win_off/d_win_len describe `nwindows` windows; job k scans
 * windows [job_start[k], job_start[k+1]) against adapter job_adapter[k] and -- when job_adapter_b
 * is non-NULL and job_adapter_b[k] >= 0 -- also against that second adapter IN THE SAME PASS (each
 * window is then read from HBM once for both).  Results, PC_RESULT_INTS each, are written in job
 * order: for job k first its n_k records for job_adapter[k], then (if any) its n_k records for
 * job_adapter_b[k].  max_len is an upper bound on every win_len (checked on the device).  The
 * arena must be readable 16 bytes past its last window (the kernels fetch 16 columns per load).  Asynchronous on `stream`; call pc_sync()
 * (or otherwise order your reads after it on the same stream) before reading d_out.
 * A context is used from ONE host thread and ONE stream at a time: its scratch (trace slab, pass-1
 * buffer, work counters) is shared by successive calls and ordered only by that stream.  Other streams
 * of the process (an upload of the next batch, say) are never synchronised with: the tile table of a call
 * is built on the context's own stream in the table slot the call before last used. */
int pc_scan_device(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off,
                   const int32_t *d_win_len, int64_t nwindows, const int32_t *job_adapter,
                   const int32_t *job_adapter_b, const int64_t *job_start, int njobs, int max_len,
                   int mode, int32_t *d_out, void *stream);

/* pc_scan_device in PC_MODE_TWO_PASS with a score floor per job (host arrays of njobs entries; job_floor_b, for the jobs'
 * second adapters, may be NULL when job_adapter_b is): a caller that only wants the alignments whose score can reach some
 * bound -- Pipeline.phase_c keeps a middle hit only if its full-adapter identity reaches --middle_threshold, which needs
 * a score of at least Pipeline.identity_score_bound -- says so, and the library decides between its two passes: a pair
 * whose best score of the first pass is below its job's floor is not traced.  Its record is "no alignment": field 0 is
 * -1, the others 0.  Every other pair gets exactly the record pc_scan_device writes.  The second pass then costs what the
 * remaining pairs cost (they are taken first, tile by tile; tiles of skipped pairs only end at once); no host round trip and
 * no further score pass is added, only the three small launches that order the pairs.  INT32_MIN = no floor for that job; both arrays NULL, or every entry INT32_MIN, is
 * pc_scan_device itself.  Any other mode with a floor array is PC_ERR_BAD_ARG.  The floor is per call, not context state.
 * It is ignored -- every pair traced -- for jobs on the plain-int32 kernel and for a launch group of more than 256
 * (job, adapter) segments. */
int pc_scan_device_floored(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off,
                           const int32_t *d_win_len, int64_t nwindows, const int32_t *job_adapter,
                           const int32_t *job_adapter_b, const int64_t *job_start, int njobs, int max_len,
                           int mode, int32_t *d_out, void *stream, const int32_t *job_floor,
                           const int32_t *job_floor_b);

/* pc_scan_device_floored with per-call flags (0: pc_scan_device_floored itself; an unknown bit is PC_ERR_BAD_ARG).
 * PC_SCAN_NO_SKIP_UNDERFILLED: the score pass of this call skips no adapter rows (see pc_set_row_skip_debug below) in a launch
 * group that does not fill the device -- one whose windows the library cuts into column chunks.  Such a launch is made of few,
 * short units, which pay the skip's entry and exit more often than they save rows: Pipeline.phase_c sets the flag for its
 * mask-and-realign rounds.  A group that fills the device keeps the skip.  Records are the same either way.  The flag belongs
 * to the call: it is no context state and the next call knows nothing of it. */
#define PC_SCAN_NO_SKIP_UNDERFILLED 1
int pc_scan_device_floored_flags(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off,
                                 const int32_t *d_win_len, int64_t nwindows, const int32_t *job_adapter,
                                 const int32_t *job_adapter_b, const int64_t *job_start, int njobs, int max_len,
                                 int mode, int32_t *d_out, void *stream, const int32_t *job_floor,
                                 const int32_t *job_floor_b, int flags);

/* pc_scan_device over END WINDOWS with the trimming rule of their caller: phase B keeps, per read and side, the largest trim
 * among the alignments that qualify (identity above end_threshold, not flush with the window's inner edge, at least
 * min_trim_size columns), so a pair that cannot qualify need not be traced.  job_side (host, njobs entries) says what a
 * job's windows are: 0 = start windows (seq[:end_size]), 1 = end windows (seq[-end_size:]), negative = the rule does not
 * apply to the job.  The library scans every window score-only first (this call, and only this call, takes windows shorter
 * than 2 * window + 64 columns in two passes under PC_MODE_AUTO; PC_MODE_TWO_PASS is accepted too, any other mode is
 * PC_ERR_BAD_ARG), decides between the passes from each pair's score record and window length (csrc/pc_end_rule.h: one
 * round, nothing about other pairs' trims or barcode calls), answers the pairs that cannot trim with the "no alignment"
 * record (field 0 = -1, the others 0) and traces the rest as PC_MODE_TRACE_AT does, taken by end column.  Every traced pair
 * gets exactly the record pc_scan_device writes.  No host round trip.  rule == NULL and job_side == NULL is pc_scan_device
 * itself; PC_NO_END_FLOOR=1 in the environment makes every call so.  The rule is ignored -- every pair traced -- for jobs
 * on the plain-int32 kernel and for a launch group of more than 16 (job, adapter) segments. */
typedef struct pc_end_rule {
    int32_t end_size, min_trim_size, extra_end_trim;
    double end_threshold;                /* percent, as --end_threshold */
} pc_end_rule;
int pc_scan_device_end_rule(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off,
                            const int32_t *d_win_len, int64_t nwindows, const int32_t *job_adapter,
                            const int32_t *job_adapter_b, const int64_t *job_start, int njobs, int max_len,
                            int mode, int32_t *d_out, void *stream, const pc_end_rule *rule,
                            const int32_t *job_side);

/* Pairs pc_scan_device_floored or pc_scan_device_end_rule left untraced: in the last such call of this context, and in all of them.  Waits for `stream`.  Either pointer may be NULL. */
int pc_floor_skipped(pc_ctx *ctx, void *stream, int64_t *last_call, int64_t *total);

/* The score pass of pc_scan_device_floored computes the adapter rows that no alignment reaching its pair's floor can reach
 * only behind a column that announces such an alignment (csrc/pc_bounds.h, row_skip_plan): records of pairs at or above
 * their floor, pc_floor_skipped and everything pass 2 sees are what they are without it.  PC_NO_ROW_SKIP=1 in the
 * environment (read per call) switches it off.  The kernel that does it holds the shorter adapter of a pair of different
 * lengths top-aligned (row_skip_plan_top); PC_SKIP_LAYOUT=bottom, read when a kernel is first asked for, compiles the
 * bottom-aligned variant instead (A/B measurements; results are the same).  A debug switch, off by default: while it is on, every wave of such a launch
 * adds, once, two numbers to two counters of the context: the 4-column blocks its fast path ran (`column_pairs`: blocks, the
 * name is historical) and those among them in which the lower rows were computed.  A stretch of blocks entered from the
 * one-column path starts with the lower rows on whatever the reads hold; its blocks are counted only from the first one
 * that triggers or lets that first window run out, so that a tile in which nothing ever triggers counts 0 of n, not W_low / 4
 * of n per stretch.  pc_row_skip_blocks waits for `stream`, reads the counters (either pointer may be NULL) and clears them. */
int pc_set_row_skip_debug(pc_ctx *ctx, int enabled);
int pc_row_skip_blocks(pc_ctx *ctx, void *stream, int64_t *column_pairs, int64_t *lower_rows_on);

/* Alignment PATHS: pair p aligns window [d_win_off[p], + d_win_len[p]) of the arena with adapter d_adapter_idx[p] of the
 * context's table and gets its record (d_records[p][8]), a head (d_heads[p][4]) and the operations of its path
 * (d_ops[p][ops_pitch_words]).  All pointers but `ctx` are device memory; d_records and d_heads are 16-byte aligned.
 *   * The scheme is the context's; any scheme the plain-int32 arithmetic holds (pc_set_scores' condition, over windows of
 *     max_len bases) is taken, the ones the packed kernels refuse included.  n == 0 is fine.
 *   * Windows may overlap, repeat, start at any byte and be empty; only bytes inside a window are read.  max_len bounds
 *     every d_win_len[p].
 *   * ops_pitch_words >= ceil((max_len + longest adapter of the table) / 16), else PC_ERR_BAD_ARG before anything is
 *     launched.  A table holding an adapter above 128 bases is PC_ERR_BAD_ARG as well.
 *   * The adapter indices live on the device and the call makes no host round trip: an index outside the table (like a
 *     window longer than max_len) is caught by the kernel, which writes nothing for that pair, and surfaces as
 *     PC_ERR_INTERNAL at pc_sync.  Callers that hold the indices on the host check them there.
 *   * The records are exactly those pc_scan_device / pc_align_batch_host give for the same pairs.
 *   * head = {path_len, read_first, adapter_first, opens}: steps of the path, read bases before its first cell, adapter
 *     bases before it (one of the two is 0), gap steps that opened their gap.
 *   * Operations are two bits each: 0 '=' diagonal over equal Dna5 codes (N == N is equal), 1 'X' diagonal over unequal
 *     ones, 2 'I' read base against a gap, 3 'D' adapter base against a gap.  They come in TRACEBACK order, from the end
 *     cell to the path's first cell, sixteen to a dword, the first in the lowest bits; words behind the last operation are
 *     not written.  pc_path_cigar turns them around.
 *   * The trace lives in a scratch buffer of the context; a call is cut into consecutive launches, in stream order on
 *     `stream`, whose scratch stays under 256 MB each (PC_PATHS_SCRATCH_MB, read per call) but which never hold fewer than
 *     64 pairs.  Asynchronous; an inconsistency surfaces as PC_ERR_INTERNAL at pc_sync, as for the scans. */
int pc_align_paths(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                   const int32_t *d_adapter_idx, int64_t n, int max_len, int32_t *d_records, int32_t *d_heads,
                   uint32_t *d_ops, int64_t ops_pitch_words, void *stream);
/* Host: (ops, path_len) of one pair -> the forward run-length string ("17=1X4=2I6="), NUL-terminated when it fits in
 * buflen.  -> the length it needs, without the NUL. */
int pc_path_cigar(const uint32_t *ops, int path_len, char *buf, size_t buflen);

/* Paths of MIDDLE hits: hit h is the alignment of adapter d_adapter_idx[h] of the context's table against the trimmed read
 * [d_read_off[h], + d_read_len[h]) of the arena, MASKED as its round of mask-and-realign saw it: every base inside one of
 * the intervals d_intervals[d_mask_base[h] .. + d_mask_count[h]) reads as '-' (Dna5 code 4, like N).  d_read_end[h] is the
 * hit's exclusive read end, as the scan reported it.  Outputs are those of pc_align_paths, record, head and operations in
 * TRIMMED-READ coordinates (read_first counts from the trimmed read's first base).  All pointers but `ctx` are device
 * memory; d_records and d_heads are 16-byte aligned.
 *   * Only a window of the read is aligned: with W, SPAN and window = W + SPAN + 1 of the adapter's own length
 *     (pc_bounds.h), columns max(0, read_end - window) + 1 .. min(read_len, read_end + W).  Given the read end of an
 *     alignment the whole masked read has, record, head and operations are exactly those of pc_align_paths over the
 *     whole, explicitly masked read.  Under a scheme the packed kernels refuse the window is the
 *     whole read.  Only bytes inside the window are read.
 *   * d_intervals is int32 [n][2], {start, end (exclusive)} in trimmed-read coordinates, one row per hit of the call; a
 *     caller lists the hits sorted stably by read, so that hit h at rank k within its read has d_mask_base[h] = its
 *     read's first row and d_mask_count[h] = k.  Intervals may be empty, overlap or reach past the read.
 *   * The host knows the widest window without reading device memory (pc_middle_paths_cols): min(max_len, the largest
 *     window + W of the table), or max_len under a refused scheme.  ops_pitch_words >= ceil((that + longest adapter of
 *     the table) / 16), else PC_ERR_BAD_ARG before anything is launched.  A table holding an adapter above 128 bases is
 *     PC_ERR_BAD_ARG as well.  n == 0 is fine.
 *   * No host round trip: a hit whose d_read_len is above max_len, whose adapter index is outside the table, whose
 *     d_read_end is outside [0, d_read_len], whose d_mask_count is negative or whose interval run leaves the n rows is
 *     caught by the kernel, which writes nothing for that hit, and surfaces as PC_ERR_INTERNAL at pc_sync.  So does a
 *     d_read_end no alignment of the masked read has (the walk leaves the window).
 *   * The trace lives in a scratch buffer of the context; slicing into launches follows pc_align_paths' rule (the same
 *     PC_PATHS_SCRATCH_MB, read per call, never fewer than 64 hits).  Asynchronous. */
int pc_middle_paths(pc_ctx *ctx, const void *d_arena, const int64_t *d_read_off, const int32_t *d_read_len,
                    const int32_t *d_adapter_idx, const int32_t *d_read_end, const int64_t *d_mask_base,
                    const int32_t *d_mask_count, const int32_t *d_intervals, int64_t n, int max_len,
                    int32_t *d_records, int32_t *d_heads, uint32_t *d_ops, int64_t ops_pitch_words, void *stream);
/* Host: the widest window (columns) a hit of pc_middle_paths can have over reads of up to max_len bases with the context's
 * table and scheme; < 0: an error code. */
int pc_middle_paths_cols(pc_ctx *ctx, int max_len);

/* UMI extraction: the read bases that lie under an adapter's degenerate letters (csrc/pc_umi.h).  Window p = [d_win_off[p],
 * + d_win_len[p]) of the arena is aligned with adapter `adapter` of the context's table -- ONE adapter per call, a host
 * value -- exactly as pc_align_paths aligns it, and the path is walked on the device: no operation leaves it.  All
 * pointers but `ctx` and `rule` are device memory; d_records and d_umi are 16-byte aligned.
 *   * The adapter's UMI span is rows u0 .. u1 (pc_umi_span): its first and last row whose letter set holds two or more
 *     bases.  Walking the path forward, a window column belongs to the UMI when a diagonal step consumes it with a span
 *     row, or an insertion consumes it with a span row behind it and one still ahead (u0 < next row <= u1).  These columns
 *     are one run [first, first + len); covered = the diagonal steps among them.
 *   * d_records[p][8] is the record pc_scan_device writes for the pair.  d_umi[p] = {status, first, len, covered}:
 *       0  complete: the path starts at or before row u0 and consumes row u1 or one behind it
 *       1  no alignment (the record's field 0 < 0; an empty window included)
 *       2  the alignment does not qualify under `rule` for a window of side `side` (0: start windows, 1: end windows):
 *          phase B's condition for a trim -- identity above end_threshold, read_end - read_start >= min_trim_size, not
 *          flush with the window's inner edge (side 0: read_end != end_size; side 1: read_start != 0).  rule == NULL:
 *          every alignment qualifies.  extra_end_trim is not read.
 *       3  the window's edge clipped the span: first, len and covered describe the part that is there
 *     Statuses 1 and 2 have first = -1, len = covered = 0; so has a span with no column under it (len == 0).
 *   * LDS and scratch are sized from THIS adapter's rows, not from the table's longest.  Trace and operations live in
 *     scratch buffers of the context; slicing into launches follows pc_align_paths' rule (PC_PATHS_SCRATCH_MB, read per
 *     call, never fewer than 64 pairs).
 *   * PC_ERR_BAD_ARG before anything is launched: an adapter index outside the table, an adapter above 128 rows, an
 *     adapter without a span, wildcards off (pc_set_wildcards), a side outside 0..1, n < 0.  n == 0 is a no-op.
 *   * No host round trip; asynchronous on `stream`.  A window above max_len and a walk that leaves its operations are
 *     caught by the kernel, which writes nothing for that pair, and surface as PC_ERR_INTERNAL at pc_sync. */
int pc_umi_extract(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len, int64_t n,
                   int max_len, int adapter, int side, const pc_end_rule *rule, int32_t *d_records, int32_t *d_umi,
                   void *stream);
/* Host: the UMI span of adapter `adapter` under the context's letter rule.  -> 1 and *first, *last (0-based rows,
 * inclusive; either pointer may be NULL), 0 if the adapter has no span (wildcards off included; *first = *last = -1),
 * PC_ERR_BAD_ARG for an index outside the table. */
int pc_umi_span(pc_ctx *ctx, int adapter, int *first, int *last);

/* UMI neighbours: which of n keys lie within max_dist edits of one another (csrc/pc_umi_dist.h, csrc/pc_umi_groups.hip) --
 * the all-against-all pass behind UMI groups.  All pointers but `ctx` are device memory.
 *   * Key k is up to 64 bases as two bit planes d_planes[k] = {p0, p1} and a length d_len[k]: base t has code c (A C G T/U =
 *     0 1 2 3), bit t of p0 is c & 1, bit t of p1 is c >> 1.  Plane bits at and above the length are ignored.
 *   * Every pair i < j whose unit-cost edit distance (Levenshtein) is <= max_dist is reported ONCE as d_pairs[slot] =
 *     {i, j, distance}, in no particular order.  *d_found is zeroed by the call on `stream` and counts ALL such pairs; only
 *     those that draw a slot below `cap` are written.  *d_found > cap therefore means the list is INCOMPLETE: call again
 *     with cap >= *d_found.  An incomplete list must never be consumed as proof that a key has no neighbour.
 *   * max_len bounds the lengths: <= 32 runs the 32-bit kernel, anything else the 64-bit one.  A key whose length is
 *     outside 0 .. max_len has no pairs, is counted in the context's error word and surfaces as PC_ERR_INTERNAL at pc_sync.
 *   * PC_ERR_BAD_ARG before anything is launched: n < 0, n > 2^31 - 1, max_len or max_dist outside 0 .. 64, cap < 0, d_found
 *     NULL.  n < 2 zeroes *d_found and launches nothing else.
 *   * Nothing outside the three input arrays is read; every index and the counter are 64-bit; no host round trip;
 *     asynchronous on `stream`.  PC_UMI_NO_PRUNE=1 (read per call) runs the DP for every pair instead of settling most of
 *     them by the lower bound: the same pairs, for tests and measurements. */
int pc_umi_neighbours(pc_ctx *ctx, const uint64_t *d_planes, const int32_t *d_len, int64_t n, int max_len, int max_dist,
                      int32_t *d_pairs, int64_t cap, int64_t *d_found, void *stream);

/* UMI neighbours over BOTH STRANDS of a molecule: pc_umi_neighbours' contract -- the same arguments, checks, counter, cap and
 * PC_UMI_NO_PRUNE -- except that a pair is FOUR int32, d_pairs[slot] = {i, j, d, flip} (d_pairs holds 4 * cap of them):
 *   * mirror(key) is the key of the reverse complement: base t of it is 3 - base(len - 1 - t) (csrc/pc_umi_dist.h).  A read of
 *     the other strand of a molecule shows the key START+END as rc(END)+rc(START) = mirror(START+END).
 *   * d = min(d_same, d_mirror) with d_same the edit distance of key i and key j and d_mirror that of key i and mirror(key j)
 *     (= that of mirror(key i) and key j); flip = 1 iff d_mirror < d_same, a tie gives 0.  The pair i < j is reported once iff
 *     d <= max_dist, and d and flip are exact whenever it is.  A key is never paired with itself. */
int pc_umi_neighbours_stranded(pc_ctx *ctx, const uint64_t *d_planes, const int32_t *d_len, int64_t n, int max_len, int max_dist,
                               int32_t *d_pairs, int64_t cap, int64_t *d_found, void *stream);

/* UMI consensus, one round: every member of every group is aligned to its group's template, the alignments vote, the votes
 * are called (csrc/pc_consensus.h states the rule, csrc/pc_consensus.hip the kernels).  Arrays named h_ are HOST memory, those
 * named d_ device memory.
 *   * Group g (0 <= g < n_groups) has the template d_tmpl_arena[h_tmpl_off[g] .. + h_tmpl_len[g]) and the members
 *     h_group_first[g] .. h_group_first[g + 1] - 1 (h_group_first holds n_groups + 1 entries, from 0 up to n_members); member m
 *     is d_arena[d_member_off[m] .. + d_member_len[m]) and d_member_group[m] names its group.  All offsets are 64-bit.
 *   * Alignment: the banded global unit-cost edit distance of pc_consensus.h, 1 <= band <= 127.  Per member d_member_out[m] =
 *     {status, distance}: 0 accepted, 1 rejected (distance * 100 > max_err_pct * max(lengths); the distance is 0x3fffffff when
 *     no path stays inside the band), 2 invalid (distance -1).
 *   * d_voters[g] = accepted members + tmpl_counts (1 when the template is itself a read of the group and stands for it, 0
 *     when it is an earlier consensus).  The template votes for its own base in every column either way.
 *   * d_cons: group g's consensus starts at byte sum over h < g of (5 min(h_tmpl_len[h], max_len) + 4) -- room for the longest
 *     sequence the votes can give -- and d_cons_len[g] says how many bytes are valid.
 *   * d_votes: NULL, or the counters of ALL groups, group g's 21 la + 16 counters (la = min(h_tmpl_len[g], max_len)) behind those
 *     of the groups before it, in pc_consensus.h's layout: for tests and debugging.
 *   * Slices.  The groups are taken in slices whose votes (4 bytes a counter) and trace (members x (longest template + 1) x 64
 *     bytes) stay under 4096 MB (PC_CONSENSUS_SCRATCH_MB, read per call); a slice is never fewer than one group, and a group
 *     that alone is above the budget is refused before anything is launched: PC_ERR_OVER_BUDGET, *refused_group (when not
 *     NULL, else -1) names it.
 *   * PC_ERR_BAD_ARG before anything is launched: band outside 1 .. 127, max_len outside 1 .. 2^24, max_err_pct outside 0 .. 100,
 *     tmpl_counts outside 0 .. 1, a negative count, a template length < 1, a negative template offset, h_group_first not rising
 *     from 0 to n_members.  n_groups == 0 or n_members == 0 does nothing at all.
 *   * A template or member above max_len, a member naming a group other than the one h_group_first puts it in, or a walk that
 *     leaves its band is counted in the context's error word and surfaces as PC_ERR_INTERNAL at pc_sync; such a member is
 *     invalid and casts no vote, such a group's consensus is empty.  Nothing is read or written outside the arrays.
 *   * The call waits for `stream` first (its scratch may still serve the call before), then enqueues and returns. */
int pc_consensus_round(pc_ctx *ctx, const void *d_arena, const void *d_tmpl_arena, const int64_t *h_tmpl_off, const int32_t *h_tmpl_len,
                       const int64_t *h_group_first, int64_t n_groups, const int64_t *d_member_off, const int32_t *d_member_len,
                       const int32_t *d_member_group, int64_t n_members, int band, int max_err_pct, int max_len, int tmpl_counts,
                       uint8_t *d_cons, int32_t *d_cons_len, int32_t *d_voters, int32_t *d_member_out, uint32_t *d_votes,
                       int64_t *refused_group, void *stream);

/* pc_consensus_round with a strand per member: d_member_strand[m] (device memory, n_members bytes) != 0 reads member m as its
 * REVERSE COMPLEMENT -- its base j is the complement of d_arena[d_member_off[m] + d_member_len[m] - 1 - j]: A <-> T, C <-> G, U
 * as T, any other byte stays a byte that matches nothing and casts no vote.  The member's bytes are not changed; alignment,
 * votes and call are those of the materialised reverse complement, in the template's coordinates.  Templates are never
 * flipped: a caller that wants a consensus in the other orientation reverse-complements it on the host.  d_member_strand NULL
 * means all 0, and that call IS pc_consensus_round: the same kernels, the same bytes.  Everything else as above. */
int pc_consensus_round_stranded(pc_ctx *ctx, const void *d_arena, const void *d_tmpl_arena, const int64_t *h_tmpl_off,
                                const int32_t *h_tmpl_len, const int64_t *h_group_first, int64_t n_groups, const int64_t *d_member_off,
                                const int32_t *d_member_len, const int32_t *d_member_group, const uint8_t *d_member_strand,
                                int64_t n_members, int band, int max_err_pct, int max_len, int tmpl_counts, uint8_t *d_cons,
                                int32_t *d_cons_len, int32_t *d_voters, int32_t *d_member_out, uint32_t *d_votes, int64_t *refused_group,
                                void *stream);

/* pc_consensus_round_stranded (d_member_strand may be NULL) that also leaves ONE QUALITY VALUE PER CONSENSUS BYTE.
 *   * h_qtab: 256 HOST bytes, each 0 .. 93 (Phred, not ASCII), consumed before the call returns.  d_qual: device memory laid out
 *     exactly like d_cons -- group g starts at the same byte, and d_cons_len[g] bytes are valid.
 *   * d_qual[byte] = h_qtab[min(margin, 255)], margin the VOTE MARGIN of the base at that byte (csrc/pc_consensus.h:
 *     column_margin, slot_margin; integers only).  Column whose call is base b: with c the five counters as the call sees them
 *     (the template's own vote included) and e = c, less one for the template's base when tmpl_counts == 0 (an earlier
 *     consensus decides ties but is no evidence), margin = max(0, e[b] - max over k != b of e[k]), deletion among the k.
 *     Insertion slot emitted with base b: with cnt its four counters and absent = d_voters[g] - their sum, margin = max(0,
 *     cnt[b] - max(absent, max over k != b of cnt[k])).  A column where deletion leads and a slot that is not emitted have no
 *     byte and no quality; which bases are emitted, and their order, are those of pc_consensus_round_stranded.
 *   * PC_ERR_BAD_ARG before anything is launched: a table entry above 93, or exactly one of h_qtab and d_qual NULL.  With both
 *     NULL the call IS pc_consensus_round_stranded: the same kernels, the same bytes.
 *   * Slices, the scratch budget, PC_ERR_OVER_BUDGET, the error word and everything else as above. */
int pc_consensus_round_quality(pc_ctx *ctx, const void *d_arena, const void *d_tmpl_arena, const int64_t *h_tmpl_off,
                               const int32_t *h_tmpl_len, const int64_t *h_group_first, int64_t n_groups, const int64_t *d_member_off,
                               const int32_t *d_member_len, const int32_t *d_member_group, const uint8_t *d_member_strand,
                               int64_t n_members, int band, int max_err_pct, int max_len, int tmpl_counts, uint8_t *d_cons,
                               int32_t *d_cons_len, int32_t *d_voters, int32_t *d_member_out, uint32_t *d_votes, int64_t *refused_group,
                               void *stream, const uint8_t *h_qtab, uint8_t *d_qual);

/* Load-balancing hint for the whole-read scans of the following pc_scan_device calls: the typical
 * (mean) window length, when max_len is far above it -- real read sets are log-normal, the longest read
 * tens of times the mean.  The score pass then cuts every window into column chunks about that long,
 * hands them to the chip longest window first and lets workgroups draw further chunks as they finish,
 * so a launch no longer lasts as long as its longest read.  0 (the default) = lengths are about uniform.
 * Affects scheduling only, never results (the chunked pass is exact, pc_bounds.h). */
int pc_set_length_hint(pc_ctx *ctx, int typical_len);

/* Kernel-variant switch for cross-checks: enabled != 0 makes every later launch of this context use the packed-int16
 * kernels (21 / 6 ops per cell pair) even where the packed-fp16 ones (13.25 / 5) are proven exact by the host gates
 * of csrc/pc_bounds.h.  Results are bit-identical either way -- that is what a cross-check of the two asserts
 * (bench.py's device_crosscheck leg, tests/test_gpu_parity.py).  Default 0; PC_DISABLE_F16=1 / PC_JIT_INT16=1 in the
 * environment force the same process-wide. */
int pc_set_int16_only(pc_ctx *ctx, int enabled);

/* Waits for `stream` and returns PC_ERR_INTERNAL if any kernel since the last pc_sync reported
 * an inconsistency. */
int pc_sync(pc_ctx *ctx, void *stream);

/* Kernel timing hooks (bench.py roofline leg): when enabled, every kernel launch made by
 * pc_scan_device is bracketed by HIP events on the launch stream.  pc_get_timing waits for the
 * stream, then returns per kernel kind (0 = generic score-only scan, 1 = window planner, 2 = traced
 * scan, 3 = run-time specialised score-only scan, 4 = exact prefilter: all its launches and its one host round trip,
 * 5 = the prefilter's seed scan alone, a sub-interval of 4 whose "pairs" are windows, 6 = the selection kernels of
 * phase B's exact pruning: pc_phase_b_select / _gather / _scatter) the summed duration in milliseconds, the number
 * of launches and the number of pairs they covered, and resets the accumulators.  Each array
 * holds PC_KERNEL_KINDS entries. */
/* (PC_KERNEL_KINDS grew from 4 to 7 in round 3: a caller built against the older header must enlarge its three arrays.) */
#define PC_KERNEL_KINDS 7
int pc_set_timing(pc_ctx *ctx, int enabled);
int pc_get_timing(pc_ctx *ctx, void *stream, double *ms, int64_t *launches, int64_t *pairs);

/* Per-read reduction of end-window records on the device -- what porechop/nanopore_read.py:166-208
 * (find_start_trim / find_end_trim) and :399-466 (determine_barcode, without the Albacore rule) do per
 * read, for a whole batch.  d_records: the records pc_scan_device wrote for njobs jobs over the SAME n
 * reads; job j = one adapter sequence against every read's start (job_side[j] = 0) or end (1) window,
 * its record for read r at d_records[(job_record_offset[j] + r) * PC_RESULT_INTS].  Writes
 * d_start_trim[n] / d_end_trim[n]: the largest trim any alignment justifies (aligned identity >
 * end_threshold, not touching the window's inner edge, at least min_trim_size bases; + extra_end_trim).
 * nbins > 0 additionally calls barcodes: bin k's start / end entry is job bin_start_job[k] /
 * bin_end_job[k] (-1 = none, scores 0.0) and d_call[r] becomes the bin index or -1 ('none') by the
 * reference's rules, ties resolved like Python's stable sort (earlier entry wins; start entries
 * before end entries).  Identities are the %f-rounded doubles Python parses.  Host arrays are copied
 * before the call returns; asynchronous on `stream`. */
int pc_phase_b_reduce(pc_ctx *ctx, const int32_t *d_records, int64_t n, int njobs,
                      const int64_t *job_record_offset, const int32_t *job_side, int end_size,
                      int min_trim_size, int extra_end_trim, double end_threshold,
                      int32_t *d_start_trim, int32_t *d_end_trim, int nbins,
                      const int32_t *bin_start_job, const int32_t *bin_end_job,
                      double barcode_threshold, double barcode_diff, int require_two_barcodes,
                      int32_t *d_call, void *stream);

/* pc_phase_b_reduce for records most of which are PC_MODE_SCORE records left untraced by the exact pruning below:
 * d_traced_mask[njobs][(n + 63) / 64] (bit r % 64 of word r / 64 of row j) says which pairs hold a traced record -- the union
 * of the selection rounds' masks; a pair whose bit is clear is read as "no alignment" without its record being loaded (the
 * reduction would skip it anyway: 94 % of the records of a barcoded batch).  NULL = pc_phase_b_reduce. */
int pc_phase_b_reduce_masked(pc_ctx *ctx, const int32_t *d_records, int64_t n, int njobs,
                             const int64_t *job_record_offset, const int32_t *job_side, int end_size,
                             int min_trim_size, int extra_end_trim, double end_threshold,
                             int32_t *d_start_trim, int32_t *d_end_trim, int nbins,
                             const int32_t *bin_start_job, const int32_t *bin_end_job,
                             double barcode_threshold, double barcode_diff, int require_two_barcodes,
                             int32_t *d_call, const uint64_t *d_traced_mask, void *stream);

#define PC_EXPLAIN_INTS 12
/* WHY pc_phase_b_reduce trimmed and called a read as it did: the per-read data the reference keeps in
 * start_adapter_alignments / end_adapter_alignments and best / second-best barcodes (nanopore_read.py:178-183,200-205,
 * 399-416), as arrays.  Every input means what it means for pc_phase_b_reduce[_masked]: record layout, job order, side,
 * absent bins (-1), untraced pairs (d_traced_mask, may be NULL), -1 / -2 records read as "no alignment", identities as
 * the %f-rounded doubles.  Two passes over the same records:
 *
 * SUMMARY pass (d_hit_first == NULL) writes d_summary[n][PC_EXPLAIN_INTS] and d_bscore[n][4]:
 *   [0], [1]   start and end trim -- equal to what pc_phase_b_reduce writes
 *   [2], [3]   number of qualifying start / end alignments: aligned identity > end_threshold, read_end - read_start >=
 *              min_trim_size, and read_end != end_size (start side) / read_start != 0 (end side)
 *   [4], [5]   deciding start / end job: the FIRST job in job order whose trim equals the read's trim; -1 when no
 *              alignment raised the trim above 0
 *   [6], [7]   best and second-best start bin, [8], [9] the same for the end side; -1 = 'none'
 *   [10], [11] reserved, 0
 *   d_bscore   the full-adapter identities of [6] .. [9], 0.0 beside a -1
 * Best and second best are the first two entries of Python's stable descending sort of that side's PRESENT entries:
 * among equal scores the earlier bin wins; a side with fewer than one / two present entries gives -1 with 0.0; an
 * absent (bin job -1) or untraced entry is never listed, while a present failed alignment is listed with 0.0.
 * nbins <= 0: [6] .. [9] are -1 and the scores 0.0.
 *
 * FILL pass (d_hit_first given: [n + 1], the exclusive prefix sum of [2] + [3] over the reads, with the total in
 * entry n) reads d_summary (field [2]) and writes read r's qualifying alignments to rows d_hit_first[r] ... of
 * d_hits[total][6]: its start alignments in job order, then its end alignments in job order -- the order the reference
 * appends them.  A row is {job, read_start, read_end (exclusive), matches, aligned_len, full_len}; the two identities
 * of the reference's tuple are 100 * matches / aligned_len and / full_len, rounded like every identity here.  A row
 * beyond d_hit_first[r + 1] is not written.  d_bscore may be NULL in this pass.
 * Alignment: d_records, d_summary and d_bscore must be 16-byte aligned (rows are read and written 16 bytes at a time),
 * d_hits 8-byte aligned.
 *
 * Under the exact pruning below the non-deciding alignments and the second-best barcode are deliberately left
 * untraced: full lists need records in which every pair is traced.  Host arrays are copied before the call returns;
 * asynchronous on `stream`. */
int pc_phase_b_explain(pc_ctx *ctx, const int32_t *d_records, int64_t n, int njobs,
                       const int64_t *job_record_offset, const int32_t *job_side, int end_size,
                       int min_trim_size, int extra_end_trim, double end_threshold, int nbins,
                       const int32_t *bin_start_job, const int32_t *bin_end_job,
                       const uint64_t *d_traced_mask, int32_t *d_summary, double *d_bscore,
                       const int64_t *d_hit_first, int32_t *d_hits, void *stream);

/* Exact pruning of phase B: of the ~200 end-window alignments a barcoded read gets, two or three decide its trims and
 * its barcode call; a score-only pass (PC_MODE_SCORE, 5 instead of 13.25 packed operations per two cells, no trace)
 * gives every alignment's end cell and score, and those bound what the alignment can contribute (the bounds and
 * their derivation: porechop_amd/csrc/pc_select.hip, porechop_amd/pipeline.py).  The caller runs
 *   score scan -> select(round 1) -> gather -> traced scan of the gathered windows -> scatter -> pc_phase_b_reduce
 *              -> select(round 2) -> gather -> traced scan -> scatter -> pc_phase_b_reduce (final),
 * which yields exactly the trims and calls of tracing everything (pc_phase_b_reduce reads a score record left in
 * place as "no alignment").  All pointers are DEVICE pointers; everything is asynchronous on `stream`.
 *
 * pc_phase_b_select: d_records as for pc_phase_b_reduce, but holding PC_MODE_SCORE records (round 1) or those with
 * round 1's traced records scattered over them (round 2); d_job_adapter_len[j] the job's adapter length,
 * d_job_calls[j] != 0 if its full identity feeds a barcode call; d_start_len / d_end_len the reads' end-window
 * lengths.  call_level = barcode_threshold - barcode_diff and call_level_diff = barcode_diff (call_level >= 1e8: no
 * barcode call).  Round 2 takes round 1's mask, the trims so far and d_best_full[2][n] (best traced barcode identity
 * per side, maintained by pc_phase_b_scatter; zero it before round 1).  Writes d_mask_out[njobs][(n + 63) / 64] -- bit
 * r % 64 of word r / 64 of row j: trace pair (j, r) -- and d_counts[njobs], the pairs selected per job.
 * d_ub_trim_out / d_ub_full_out (optional, round 1): the bounds themselves, [njobs][n], for tests. */
int pc_phase_b_select(pc_ctx *ctx, const int32_t *d_records, int64_t n, int njobs,
                      const int64_t *d_job_record_offset, const int32_t *d_job_side,
                      const int32_t *d_job_adapter_len, const int32_t *d_job_calls,
                      const int32_t *d_start_len, const int32_t *d_end_len, int end_size,
                      int min_trim_size, int extra_end_trim, double end_threshold, int round,
                      double call_level, double call_level_diff, const uint64_t *d_mask_prev,
                      const int32_t *d_start_trim, const int32_t *d_end_trim, const double *d_best_full,
                      uint64_t *d_mask_out, uint64_t *d_counts, int32_t *d_ub_trim_out,
                      double *d_ub_full_out, void *stream);
/* The selected pairs of a mask as the window lists of a traced scan: job j's pairs become windows
 * [d_job_first[j], d_job_first[j] + count[j]) (d_job_first = exclusive prefix sum of the counts), in no particular
 * order within the job; d_dest / d_pair_job / d_pair_read give each window's record index, job and read.  d_cursor:
 * njobs words of scratch. */
int pc_phase_b_gather(pc_ctx *ctx, const uint64_t *d_mask, int64_t n, int njobs, const int64_t *d_job_first,
                      uint64_t *d_cursor, const int64_t *d_job_record_offset, const int32_t *d_job_side,
                      const int64_t *d_start_off, const int32_t *d_start_len, const int64_t *d_end_off,
                      const int32_t *d_end_len, int64_t *d_win_off, int32_t *d_win_len, int64_t *d_dest,
                      int32_t *d_pair_job, int64_t *d_pair_read, void *stream);
/* d_out[k] = d_records[d_index[k]] (PC_RESULT_INTS each): the score records of the gathered pairs (d_index = d_dest) in the
 * order of the traced scan's windows -- what PC_MODE_TRACE_AT expects in its output buffer on entry. */
int pc_gather_records(pc_ctx *ctx, const int32_t *d_records, const int64_t *d_index, int64_t count, int32_t *d_out,
                      void *stream);
/* The traced records of the gathered windows over the score records they replace; d_best_full (may be NULL) is
 * raised to the full identity of every traced barcode pair. */
int pc_phase_b_scatter(pc_ctx *ctx, const int32_t *d_traced, int64_t count, const int64_t *d_dest,
                       const int32_t *d_pair_job, const int64_t *d_pair_read, int32_t *d_records,
                       const int32_t *d_job_side, const int32_t *d_job_calls, double *d_best_full, int64_t n,
                       void *stream);

/* Packed private copies of n windows on the device: window i of d_arena (d_src_off[i], d_len[i]) is copied
 * to d_dst + d_dst_off[i], and the bytes from its end up to d_dst_off[i+1] are set to `pad` (d_dst_off has
 * n + 1 entries).  Porechop masks every middle hit in a copy of the read and aligns again
 * (nanopore_read.py:212-243); the batch pipeline keeps such copies only for the reads that had a hit,
 * back to back whatever their lengths.  Asynchronous on `stream`. */
int pc_copy_windows(pc_ctx *ctx, const void *d_arena, const int64_t *d_src_off, const int32_t *d_len,
                    int64_t n, void *d_dst, const int64_t *d_dst_off, int pad, void *stream);

/* Reads cross PCIe at 2 bits per base (north_star: "2-bit-packed read windows"; a read set is 8 GB of bases per million
 * 8-kb reads and the link moves ~57 GB/s, so at one byte per base the upload, not the scan, bounds a run).
 * pc_pack_reads (host, all cores the caller may use: pc_io_set_thread_limit): base i of arena[0 .. nbases) -- one byte per
 * base as pc_readset_arena delivers them -- becomes bits 2*(i%4).. of packed[i/4] ((nbases + 3) / 4 bytes; keep the
 * buffer a multiple of 4 bytes long): SeqAn's Dna ordinal values, A 0, C 1, G 2, T/U 3, either case
 * (porechop/include/seqan/basic/alphabet_residue_tabs.h:113-140).  Every other byte ('N', '-', IUPAC codes ...: all of
 * them Dna5 'N' to the alignment, which is what the reference's conversion makes of them) is an EXCEPTION: code 0 in
 * the plane and its position appended to exc_pos (ascending).  *nexc = the number of exceptions; if that exceeds
 * exc_cap nothing is listed and PC_ERR_BAD_ARG is returned (call again with room for *nexc entries).
 * pc_unpack_device is the inverse on the device, into the byte arena every scan entry point takes: d_arena[i] = 'A' /
 * 'C' / 'G' / 'T', 'N' at the exceptions, then pad_bytes bytes of 'N' (the 16 readable bytes the scans need past the last
 * window, say).  Alignment-equivalent to the original bytes: Dna5(original) == Dna5(unpacked) for every base.
 * d_packed 4-byte aligned, d_arena 16-byte aligned, room for nbases + pad_bytes bytes.  HBM-bound (0.25 B in, 1 B out per
 * base), asynchronous on `stream`. */
int pc_pack_reads(const char *arena, int64_t nbases, uint8_t *packed, int64_t *exc_pos, int64_t exc_cap, int64_t *nexc);
int pc_unpack_device(pc_ctx *ctx, const void *d_packed, int64_t nbases, const int64_t *d_exc_pos, int64_t nexc,
                     void *d_arena, int pad_bytes, void *stream);

/* Exact bit-parallel prefilter of the whole-read ("middle") scan.  Porechop keeps a whole-read alignment only when
 * its full-adapter identity reaches --middle_threshold (porechop/nanopore_read.py:224-241); such an alignment has at
 * most pc_prefilter_max_edits(adapter length, threshold) non-matching columns inside the adapter's span, so the
 * adapter lies within that many unit-cost edits (substitutions, insertions, deletions; adapter global, overhanging
 * adapter bases are deletions; read local; equality of Dna5 codes, N == N, as in the reference) of a substring of
 * the read.  pc_prefilter_device decides that for every (window, adapter) pair with Myers' bit-vector algorithm,
 * one lane per (window chunk, adapter piece) (csrc/pc_prefilter.hip; the alternative the reference's README.md:355-357
 * points to).  Row w of d_mask ([nwindows][ceil(nadapters / 32)] words, written by the call) gets bit j set iff window
 * w MAY hold adapters[j] within max_edits[j] edits: always set when it does (so a pair whose bit is clear is PROVEN not
 * to be a hit, and only the survivors need the DP), never set when it does not for adapters of at most 32 bases;
 * a longer adapter is represented by its first 32 bases with the same bound when max_edits <= 8, and otherwise cut into
 * ceil(m / 32) pieces, surviving when one piece lies within floor(max_edits / pieces) edits (pigeonhole) -- a superset
 * either way.  max_edits[j] < 0 = do not filter adapter j (bit set for every non-empty window).
 * adapters[] indexes the table of pc_set_adapters; max_len bounds every win_len (a longer window is flagged on the
 * device and reported by pc_sync as PC_ERR_INTERNAL: its tail would otherwise go unscanned and look "proven"); the arena
 * must be readable 16 bytes past its last window, and -- because the kernels fetch whole aligned 16-byte blocks
 * (exhaustive kernel) and 128-byte lines (seed scan) -- from the 128-byte boundary at or below d_arena: d_arena itself
 * should be 128-byte aligned (hipMalloc and torch allocations are 256-byte aligned), or sit inside an allocation that
 * starts at or below that boundary.  Asynchronous on `stream`; honours pc_set_length_hint. */
int pc_prefilter_max_edits(int adapter_len, double threshold_percent);
int pc_prefilter_device(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                        int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits,
                        int nadapters, uint32_t *d_mask, void *stream);

/* The prefilter over reads held at 2 BITS PER BASE (north_star: "2-bit-packed read windows"): d_plane is pc_pack_reads' plane
 * in HBM -- a quarter of the bytes of the one HBM-bound kernel of the path, and sixteen bases ARE a dword: no byte -> code
 * step, one funnel shift per q-gram (csrc/pc_prefilter.hip seed_scan_packed_kernel) -- d_win_off counts BASES of the plane.
 * Same mask, same meaning.  Bases that were not A/C/G/T/U sit in the plane as 'A' and the exception list is NOT consulted:
 * against adapters made of A/C/G/T(U) that can only ADD survivors, so a cleared bit is still a proof.  The route takes only
 * such adapters, and only where the seed stage covers every piece (parts of >= 6 bases): otherwise
 * PC_ERR_UNSUPPORTED_SCORES -- unpack the reads (pc_unpack_device) and call pc_prefilter_device.  d_plane 16-byte aligned
 * and readable 64 bytes past its last base.
 * pc_unpack_windows: n windows of the plane (d_src_off in bases, ascending, not overlapping; d_len) as bytes -- 'A' 'C' 'G' 'T',
 * 'N' at the exceptions -- window i at d_dst + d_dst_off[i], padded with `pad` up to d_dst_off[i + 1] (d_dst_off has n + 1
 * entries).  What a run that keeps its reads packed unpacks: the 150-base end windows of every read and the whole of the
 * few reads that survive the prefilter. */
int pc_prefilter_packed(pc_ctx *ctx, const void *d_plane, const int64_t *d_win_off, const int32_t *d_win_len,
                        int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits,
                        int nadapters, uint32_t *d_mask, void *stream);

/* pc_prefilter_packed for EVERY adapter list and every bound: same arguments, same mask, never PC_ERR_UNSUPPORTED_SCORES.
 * Pieces the seed stage covers take it as above; every other piece -- parts shorter than 6 bases (--middle_threshold below
 * about 87 for a 28-mer), more than 8 parts, an adapter with a letter other than A/C/G/T/U (taken whole) -- runs Myers'
 * recurrence over every column of the plane (csrc/pc_prefilter.hip prefilter_packed_kernel: 64 bases per 16-byte fetch, the
 * Eq row picked by the 2-bit code), and so does a batch whose candidate list overflowed, immediately or on the repeat call
 * after pc_prefilter_overflowed.  Bases that were not A/C/G/T/U sit in the plane as 'A' and the exception list is NOT
 * consulted; adapter letters that are not A/C/G/T/U are wildcards in that kernel (they match all four codes), so every
 * column that matches in the reference's sense (equal Dna5 codes, N == N) still matches: a cleared bit is still a proof.
 * For adapters of A/C/G/T/U over reads without exceptions the mask equals pc_prefilter_device's over the unpacked bytes
 * bit for bit; otherwise it is a superset of it. */
int pc_prefilter_packed_any(pc_ctx *ctx, const void *d_plane, const int64_t *d_win_off, const int32_t *d_win_len,
                            int64_t nwindows, int max_len, const int32_t *adapters, const int32_t *max_edits,
                            int nadapters, uint32_t *d_mask, void *stream);

/* The seed stage sizes its verification launch from a count it reads back from the device: ONE host round trip per call.
 * pc_prefilter_defer_count(ctx, 1) removes it -- the verification is launched for the whole candidate list (threads beyond
 * the count leave at once) and the count follows to pinned host memory; after the caller's next synchronisation of the
 * stream, pc_prefilter_overflowed(ctx) says whether the last call's list overflowed (1: its mask is NOT complete -- repeat
 * the call with the deferral off; rare: low-complexity reads against a low-complexity seed). */
/* The glue of the middle scan (porechop/nanopore_read.py:56-62,210-243 for a whole batch) as single launches -- as torch
 * expressions it is ~150 launches of a few microseconds per step, and the GPU idles between them.  All pointers: device memory.
 * pc_trim_windows: seq[start_trim : len - end_trim] with Python's slice semantics -> toff / tlen; stats int64[4] = reads with a
 *   non-empty interval, longest, 2^40 - shortest non-empty (0: none), sum.
 * pc_middle_hits: full-adapter identity (the %f-printed double) of whole-read records and whether it reaches the threshold.
 * pc_group_survivors: cand[g][w] = (mask row w AND gmask row g) != 0 over the prefilter's mask, counts[g] = how many.
 * pc_round_consume: per active masked read the first adapter >= its cursor whose record is a hit; stats int64[4] = alignments
 *   consumed, reads that hit, 2^40 - smallest hit adapter (0: none), bases to mask.
 * pc_round_select: behind pc_round_consume, with its d_anyh and d_a_hit: which adapter SETS the next round must scan for
 *   which of the reads that hit.  d_set_of int32[nadapters]: the dense index (0 .. nsets - 1) of every middle adapter's set.
 *   A read's hit interval is masked, and csrc/pc_mask_rule.h says which of its records the mask can have changed:
 *   d_need[s * nact + k] = 1 when some adapter of set s at or above read k's hit adapter is the hit itself or has such a
 *   record, else 0 (reads without a hit: 0); d_counts int64[nsets] = reads that need set s.  floored_positive: the rounds'
 *   scans are floored with floors all > 0 (then a "no alignment" record is stable).  The caller decides whether the rule
 *   may be used at all (pc_mask_rule_gate).  d_counts may lie behind pc_round_consume's d_stats in one buffer, so that one
 *   copy brings both to the host. */
int pc_trim_windows(pc_ctx *ctx, const int64_t *d_off, const int32_t *d_len, const int32_t *d_start_trim, const int32_t *d_end_trim,
                    int64_t n, int64_t *d_toff, int32_t *d_tlen, int64_t *d_stats, void *stream);
int pc_middle_hits(pc_ctx *ctx, const int32_t *d_records, int64_t n, double threshold, double *d_full, uint8_t *d_hit, void *stream);
int pc_group_survivors(pc_ctx *ctx, const int32_t *d_mask, int64_t n, int words, const int32_t *d_gmask, int ngroups, uint8_t *d_cand,
                       int64_t *d_counts, void *stream);
int pc_round_consume(pc_ctx *ctx, const double *d_full_all, const int32_t *d_rec_all, const int64_t *d_cur, const int64_t *d_act,
                     int64_t nact, int nadapters, int64_t ndirty, double threshold, uint8_t *d_anyh, int32_t *d_a_hit, int64_t *d_cnt,
                     int64_t *d_stats, void *stream);

int pc_round_select(pc_ctx *ctx, const int32_t *d_rec_all, const int64_t *d_act, const uint8_t *d_anyh, const int32_t *d_a_hit,
                    const int32_t *d_set_of, int64_t nact, int nadapters, int64_t ndirty, int nsets, int floored_positive,
                    uint8_t *d_need, int64_t *d_counts, void *stream);
/* The rule's gate and the rule itself as the host compiles them (csrc/pc_mask_rule.h); no context, no device.
 * pc_mask_rule_gate: 1 when every adapter (NUL-terminated) holds A/C/G/T/U only, wildcards are off and mismatch <= match. */
int pc_mask_rule_gate(const char *const *adapters, int nadapters, int match, int mismatch, int gap_open, int gap_extend, int wildcards);
int pc_mask_rule_must_realign(int adapter, int cur, int32_t read_start, int32_t read_end, int32_t mask_start, int32_t mask_end,
                              int floored_positive);

int pc_prefilter_defer_count(pc_ctx *ctx, int enabled);
int pc_prefilter_overflowed(pc_ctx *ctx);
int pc_unpack_windows(pc_ctx *ctx, const void *d_plane, const int64_t *d_exc_pos, int64_t nexc, const int64_t *d_src_off,
                      const int32_t *d_len, int64_t n, void *d_dst, const int64_t *d_dst_off, int pad, void *stream);

/* Adapter discovery: the k-mer census of a set of windows (csrc/pc_discover.hip).  For every position p of every window
 * with p + k <= d_win_len[i], d_counts[code] += 1, where code holds the k bases from p on at 2 bits each, the FIRST base
 * in the highest bits, in SeqAn's Dna order: A 0, C 1, G 2, T 3, U as T, either case -- the byte -> code table of the
 * scans (porechop/include/seqan/basic/alphabet_residue_tabs.h:113-140).  A k-mer that covers any other byte ('N', '-',
 * IUPAC codes: all Dna5 'N') is not counted.  d_counts is the caller's dense uint32[4^k] table (4 <= k <= 13, else
 * PC_ERR_BAD_ARG and nothing is launched; 268 MB at k = 13).  The call only ADDS: one table takes block after block of a
 * streamed file; the caller zeroes it before the first.  Windows are described as for every scan (d_win_off int64 byte
 * offsets into d_arena, d_win_len int32); they may start at any byte, overlap, repeat, and be shorter than k (such a
 * window adds nothing); n = 0 is a no-op.  The arena is read as aligned dwords: only dwords that hold a byte of a window,
 * so d_arena need only sit in an allocation that starts and ends on a 4-byte boundary.  Counters wrap at 2^32.
 * Asynchronous on `stream`. */
int pc_kmer_count(pc_ctx *ctx, const void *d_arena, const int64_t *d_win_off, const int32_t *d_win_len, int64_t n, int k,
                  uint32_t *d_counts, void *stream);

/* The entries of such a table with d_counts[code] >= min_count, as a list: entry i = (d_codes[i], d_cnt[i]), in no
 * particular order, at most `cap` of them (cap >= 0; d_codes / d_cnt may be NULL when cap is 0).  *d_found (device memory,
 * set by the call) = the number of qualifying entries WHETHER OR NOT they fitted: d_found[0] > cap means the list is
 * incomplete -- call again with room for d_found[0] entries.  The call itself makes no host round trip; the caller
 * reads d_found after synchronising the stream.  k as for pc_kmer_count.  Asynchronous on `stream`. */
int pc_kmer_select(pc_ctx *ctx, const uint32_t *d_counts, int k, uint32_t min_count, int32_t *d_codes, uint32_t *d_cnt,
                   int64_t cap, int64_t *d_found, void *stream);

/* Barcode discovery: the bases next to an aligned anchor, one code per window (csrc/pc_discover.hip, insert_code_kernel).
 * d_records holds the n scan records (PC_RESULT_INTS each, window order) of ONE adapter -- the anchor, anchor_len bases --
 * against the n windows (d_win_off / d_win_len over d_arena, as for every scan); side 0: start windows, the insert lies
 * behind the anchor; side 1: end windows, it lies before it.  Window w is ANCHORED iff all of
 *   rec[0] >= 0                                   (not the "no alignment" record)
 *   rec[7] > 0
 *   100 * rec[5] >= min_identity * rec[7]         (matches and full length, integers, products in 64 bits)
 *   side 0: rec[3] == anchor_len - 1; side 1: rec[2] == 0      (the alignment reaches the anchor's inner edge)
 * The insert's first column is col = rec[1] + 1 (side 0) or rec[0] - insert_len (side 1); read coordinates in records are
 * inclusive.  d_codes[w] = the 2-bit code of the window's bytes [col, col + insert_len): the first base in the highest
 * bits, A C G T/U = 0 1 2 3, either case -- pc_kmer_count's byte -> code function -- when the window is anchored, col >= 0
 * and col + insert_len <= d_win_len[w]; otherwise, and when any of those bytes is not a base, -1.  (At insert_len = 32
 * the code fills all 64 bits: an insert that begins with G or T is a negative number, and 32 T's are -1 itself.  Callers
 * that tell inserts from -1 by sign stay at 31 or below, as discover() does.)  Nothing outside [d_win_off[w],
 * d_win_off[w] + d_win_len[w]) is read, byte by byte, and every index is formed in 64 bits; windows may overlap, repeat, be
 * empty and start at any byte.  n = 0 is a no-op.  insert_len outside 1..32, side outside 0..1, min_identity outside
 * 0..100 or anchor_len < 1 is PC_ERR_BAD_ARG before anything is launched.  No host round trip; asynchronous on `stream`. */
int pc_anchor_inserts(pc_ctx *ctx, const uint8_t *d_arena, const int64_t *d_win_off, const int32_t *d_win_len,
                      const int32_t *d_records, int64_t n, int anchor_len, int side, int min_identity, int insert_len,
                      int64_t *d_codes, void *stream);

/* Debug builds of the 16-bit kernels (PC_CHECK_RANGE=1: packed-fp16 traced kernel, every row class it has;
 * PC_JIT_CHECK_RANGE=1: the run-time specialised score kernel) record the extremes of every DP value they
 * hold, in the kernel's own offset coordinates; this returns them since the last call and resets.  The
 * exactness argument needs |value| <= 2040 in the fp16 kernels and <= 32000 in the int16 ones. */
int pc_debug_value_range(pc_ctx *ctx, int32_t *lo, int32_t *hi);

/* Packed VALU operations per TWO DP cells, times 100, of the traced end-window kernel this context's
 * scoring scheme selects (2100: packed-int16 kernel; 1325: packed-fp16 kernel) -- the denominator
 * of the VALU roofline bench.py reports. */
int pc_trace_ops_x100(pc_ctx *ctx);

/* Run-time specialised score kernels are compiled (hiprtc) once an adapter pair's accumulated work
 * pays for it.  By default the compile happens in place, inside the pc_scan_device call that
 * crosses the threshold -- provided that call alone is large enough to be worth the stall; a small
 * launch that merely tips the running total over never waits.  With pc_jit_async(1) every compile
 * runs on a worker thread and launches keep using the generic kernels until the kernel is ready --
 * no stall for one-shot runs.  Process-wide. */
void pc_jit_async(int enabled);
/* With asynchronous specialisation on, call this before the process exits: it drops compiles that
 * have not started and waits for the one in flight (a worker thread must not be inside hiprtc while
 * the process image is torn down).  The Python binding registers it with atexit. */
void pc_jit_shutdown(void);

/* Specialised kernels are pure functions of (kernel source, adapter pair's row pattern, scoring scheme): their code
 * objects are kept on disk and loaded instead of compiled -- from <directory of this library>/kernel_cache (filled
 * when the library is built: every set of the static panel, porechop/adapters.py:77-463, under the default scheme)
 * and from PC_JIT_CACHE_DIR / $XDG_CACHE_HOME/porechop_amd / ~/.cache/porechop_amd (what this machine compiled at
 * run time; PC_JIT_CACHE_DIR=off disables it).  A kernel found on disk is used from the first launch on.
 * pc_jit_precompile builds the kernel that scans adapter_a and adapter_b in one pass (adapter_b NULL or "": a alone)
 * into cache_dir (NULL or "": the in-tree directory).  It needs hiprtc but NO device.  Returns 0 = compiled and
 * written, 1 = already there, < 0 = this pair / scheme has no specialised kernel, or the compile or write failed. */
int pc_jit_precompile(const char *adapter_a, const char *adapter_b, int match, int mismatch, int gap_open,
                      int gap_extend, const char *cache_dir);
/* The pair's second kernel, which the score pass of pc_scan_device_floored runs where the pair has one: its fast path
 * computes the adapter rows below a row r0 only where an alignment that reaches the launch's floors can be (see
 * pc_set_row_skip_debug above).  Same arguments and answers; 2 = the pair has no such kernel (packed int16 lanes, or no
 * row that would pay). */
int pc_jit_precompile_row_skip(const char *adapter_a, const char *adapter_b, int match, int mismatch, int gap_open,
                               int gap_extend, const char *cache_dir);
/* Kernels this process compiled with hiprtc / took from a kernel cache on disk so far. */
void pc_jit_stats(int64_t *compiled, int64_t *from_disk);

/* Format one result record exactly as the reference prints it; buf must hold >= 160 bytes. */
int pc_format_result(const int32_t *rec, char *buf, size_t buflen);
/* The same for n records at once: the strings back to back in buf, each followed by '\n'; *used = bytes written.
 * buflen >= 161 * n always suffices.  (The drop-in's prefetch turns millions of records into the strings the
 * reference's Python parses, porechop/nanopore_read.py:476-491: one call instead of one per record.) */
int pc_format_results(const int32_t *recs, int64_t n, char *buf, int64_t buflen, int64_t *used);

/* Prefetch memo for the per-call symbol: compute these pairs on the GPU now and remember the
 * answers, keyed by (window bytes, adapter bytes, scores), so that later adapterAlignment()
 * calls with the same arguments are lookups.  Uses the process-wide default context. */
int pc_prefetch(const char *read_arena, int64_t arena_bytes, const int64_t *win_off,
                const int32_t *win_len, const char *const *adapters, const int32_t *adapter_idx,
                int64_t npairs, int match, int mismatch, int gap_open, int gap_extend);
void pc_memo_clear(void);
/* hits, misses (single-pair launches), entries */
void pc_memo_stats(int64_t *hits, int64_t *misses, int64_t *entries);

/* ------------------------------------------------------------------------------------------
 * Part 3 -- host ingest (the row after the hot path): FASTA / FASTQ, plain or
 * gzip, parsed as porechop/misc.py:60-168 does and normalised as NanoporeRead.__init__
 * (porechop/nanopore_read.py:23-35: upper-case; U->T when U's outnumber T's; qualities padded with
 * '+'), but into ONE packed arena + offset/length tables -- the inputs of the batch API above --
 * instead of per-read Python tuples.  Host code only.
 * ------------------------------------------------------------------------------------------ */
typedef struct pc_readset pc_readset;
/* Always sets *out (so pc_readset_error can be read); free it with pc_readset_free. */
int pc_readset_load(const char *path, pc_readset **out);
void pc_readset_free(pc_readset *rs);
const char *pc_readset_error(const pc_readset *rs);
int64_t pc_readset_count(const pc_readset *rs);
int pc_readset_is_fastq(const pc_readset *rs);
/* reads back to back, 1 byte per base, followed by 64 bytes of 'N' padding; *bytes includes it */
const char *pc_readset_arena(const pc_readset *rs, int64_t *bytes);
const int64_t *pc_readset_offsets(const pc_readset *rs);
const int32_t *pc_readset_lengths(const pc_readset *rs);
const char *pc_readset_name(const pc_readset *rs, int64_t i);     /* full header, no leading marker */
/* Appends " " + text[k] to the END of the stored header of read read[k], k = 0 .. n - 1 (host; the name arena is rebuilt
 * once).  Every writer (pc_readset_write, _write_at, _write_sizes, _write_shared, pc_readset_compress) and
 * pc_readset_name then give the longer header; a piece number ("_3") still goes before the header's first space, the
 * text stays at the end.  A read named twice gets both texts, in the order given.  A read index out of range, a NULL or
 * empty text and a text holding '\n' or '\r' (a NUL ends a C string: it cannot be passed) are PC_ERR_BAD_ARG, and then
 * nothing has changed.  Pointers pc_readset_name returned before the call are stale after it. */
int pc_readset_annotate(pc_readset *rs, int64_t n, const int64_t *read, const char *const *text);
const char *pc_readset_quals(const pc_readset *rs, int64_t i);    /* FASTQ only */
int pc_readset_is_rna(const pc_readset *rs, int64_t i);
/* Several FASTQ (or several FASTA) files into ONE read set, in the order given -- the Albacore
 * directory input of porechop/porechop.py:232-259; pc_readset_file_index()[i] = which path read i
 * came from. */
int pc_readset_load_many(const char *const *paths, int npaths, pc_readset **out);
/* Streaming ingest of a plain, regular 4-line FASTQ file (or a plain FASTA file, cut where a line begins with '>'): the
 * records that start in [byte_begin, cut), where
 * cut is the first record start at or after byte_begin + target_bytes (or the end of the file); *next_begin = cut.
 * Successive calls (byte_begin = the previous *next_begin, starting at 0) yield the reads of pc_readset_load in
 * the same order, a block at a time -- so that a run's memory is bounded by its blocks and ingest, scan and
 * writing of successive blocks overlap.  Returns PC_ERR_UNSUPPORTED_SCORES ("not streamable") for gzip (see
 * pc_gzstream_* below) or an irregular record: load the whole file with pc_readset_load then. */
int pc_readset_load_segment(const char *path, int64_t byte_begin, int64_t target_bytes, int64_t *next_begin,
                            pc_readset **out);
const int32_t *pc_readset_file_index(const pc_readset *rs);

/* Worker threads the ingest / writer calls made BY THE CALLING THREAD may use from now on (0 = the default: every core
 * the process may run on -- its affinity mask, capped by the container's CPU quota and at 64).  A pipelined caller that
 * loads one block on one thread while it writes another on a second gives each its share, so that the two together do
 * not oversubscribe the cores. */
void pc_io_set_thread_limit(int nthreads);

/* Output writer: the byte-level half of nanopore_read.py:97-147 (get_fasta /
 * get_fastq) and porechop.py:607-734 (output_reads).  The caller has decided which pieces of which
 * reads go where; piece k is bases [piece_start[k], piece_start[k] + piece_len[k]) of read
 * piece_read[k] (coordinates in the whole read), written to file_paths[piece_file[k]] in the
 * order given.  piece_number[k] > 0 appends "_<number>" to the read name the way
 * add_number_to_read_name does (nanopore_read.py:494-498); piece_number may be NULL.  FASTQ:
 * "@name\nseq\n+\nquals\n" (reads that came from FASTA get '+' qualities, as NanoporeRead pads
 * them); FASTA: ">name\n" + sequence wrapped at 70.  RNA reads are written with U for T.  A path
 * of "-" is stdout.  Files are created when their first piece arrives (a bin that receives
 * nothing leaves no file, like the reference). */
int pc_readset_write(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                     const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                     const char *const *file_paths, int fastq, int64_t *bytes_written);

/* pc_readset_write for a streamed run: file_pos[f] is where file f continues (0 = create / truncate it now) and is
 * updated to where it ends.  A "-" (stdout) path is simply appended to. */
int pc_readset_write_at(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                        const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                        const char *const *file_paths, int fastq, int64_t *file_pos);

/* A sharded run (one process per GPU) over ONE plain FASTQ (or FASTA) file: every rank parses only its own byte range and
 * writes its own span of the shared output files.
 * pc_fastq_find_record: the first record start at or after byte_pos (the cut pc_readset_load_segment would choose), or the
 * file size when none is left; rank r of W takes [find(size * r / W), find(size * (r + 1) / W)).  "Not streamable" (gzip,
 * an irregular record near byte_pos) is PC_ERR_UNSUPPORTED_SCORES, as for pc_readset_load_segment.
 * pc_readset_write_sizes: the bytes pc_readset_write would put into each file, nothing written -- the ranks exchange them
 * and take the prefix sums as their positions.
 * pc_readset_write_shared: pc_readset_write_at for files other processes write disjoint spans of: opened without
 * truncation whatever the position (create / truncate them once, before any rank writes). */
int pc_fastq_find_record(const char *path, int64_t byte_pos, int64_t *record_start);
int pc_readset_write_sizes(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                           const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                           int fastq, int64_t *bytes_per_file);
int pc_readset_write_shared(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                            const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                            const char *const *file_paths, int fastq, int64_t *file_pos);

/* ---- gzip at the speed of the rest (replaces: Python's gzip module on the way in, porechop/misc.py:60-81,151-168; `pigz -p
 * <threads>` / gzip over a temporary file on the way out, porechop/porechop.py:640-651,685-729) -------------------------------
 * Output is a chain of independent gzip members of <= 65 280 input bytes, each carrying its compressed size in a 'BC' extra
 * subfield (the BGZF layout of the SAM specification, 4.1): an ordinary multi-member .gz file to gunzip / zlib / Python, and
 * one whose members any reader that knows the subfield inflates in parallel.  DEFLATE comes from libdeflate when the
 * machine has it (dlopen), else zlib.
 * pc_readset_compress: the pieces pc_readset_write would write, formatted and deflated by all cores into memory (nothing is
 *   opened); level 1..9 (<= 0: the default -- libdeflate's 3, which already makes smaller files than the zlib level 6 of
 *   gzip and pigz; zlib's 6 without libdeflate).
 * pc_gzimage_sizes / pc_gzimage_write: the bytes per file, and the image of every file written at file_pos[f] (updated) --
 *   a streamed run appends block after block, the ranks of a sharded run exchange the sizes first and write disjoint spans
 *   (shared = 1: never truncate).  Files whose image is empty are not touched.
 * pc_gz_finish: the empty last member (28 bytes) that ends such a file; creates the file when there is none.
 * pc_gzip_file: a whole file, src -> dst, all cores (single_member = 1: ONE member the way pigz builds it, which nobody can
 *   inflate in parallel -- for tests and benchmarks of the reader's route for ordinary .gz input). */
typedef struct pc_gzimage pc_gzimage;
int pc_readset_compress(const pc_readset *rs, int64_t npieces, const int64_t *piece_read, const int32_t *piece_start,
                        const int32_t *piece_len, const int32_t *piece_number, const int32_t *piece_file, int nfiles,
                        int fastq, int level, pc_gzimage **out);
int pc_gzimage_sizes(const pc_gzimage *img, int nfiles, int64_t *compressed_bytes, int64_t *plain_bytes);
int pc_gzimage_write(const pc_gzimage *img, int nfiles, const char *const *file_paths, int64_t *file_pos, int shared);
void pc_gzimage_free(pc_gzimage *img);
int pc_gz_finish(const char *path);
int pc_gzip_file(const char *src, const char *dst, int level, int single_member);

/* A gzip FASTQ file made of SIZED members (what the writer above makes; bgzip) for the ranks of a sharded run: the inflated
 * stream is addressed like a plain file -- position x lies in the member whose inflated span holds it -- so that rank r of W
 * takes the records that start in [find(total * r / W), find(total * (r + 1) / W)) and inflates only the members that hold
 * them (the counterparts of pc_fastq_find_record / pc_readset_load_segment; porechop/misc.py:151-168 is what they replace).
 * pc_gz_sized_size: the inflated size; PC_ERR_UNSUPPORTED_SCORES for a file that is not made of sized members throughout.
 * pc_gz_sized_find_record: the first record start at or after `pos` of the inflated bytes (the inflated size when none is left).
 * pc_readset_load_gz_range: the records of [begin, end), both as pc_gz_sized_find_record gives them. */
int pc_gz_sized_size(const char *path, int64_t *inflated_bytes);
int pc_gz_sized_find_record(const char *path, int64_t pos, int64_t *record_start);
int pc_readset_load_gz_range(const char *path, int64_t begin, int64_t end, pc_readset **out);

/* A gzip FASTQ file as a stream of blocks (the streamed route for .gz input): a producer thread inflates ahead of the
 * caller -- members that carry their size on several cores, members without one guessed and inflated ahead, ONE big member by
 * a single libdeflate call whose output is handed over while it appears (zlib without libdeflate) -- so that inflating block
 * k+1 overlaps parsing, scanning and writing block k.
 * pc_gzstream_next: the records that start before the first record start at or after target_bytes of the bytes not yet
 *   handed out (where pc_readset_load_segment would cut the plain file), at least min_reads of them unless the file ends
 *   first; *out = NULL and *eof = 1 after the last block.  PC_ERR_UNSUPPORTED_SCORES = "not streamable" (not gzip, not a
 *   regular 4-line FASTQ, a damaged stream): load the whole file with pc_readset_load, which reproduces the reference's
 *   behaviour and messages. */
typedef struct pc_gzstream pc_gzstream;
int pc_gzstream_open(const char *path, pc_gzstream **out);
/* One rank's share of a multi-member gzip file WITHOUT sizes (`cat *.fastq.gz`): pc_gz_member_start = the first member that
 * starts at or after compressed byte pos (validated: the stream behind the magic inflates to its end and CRC-32 / ISIZE agree;
 * the file's size when there is none); pc_gzstream_open_range = the stream of pc_gzstream_open over the members in
 * [begin, end) of the compressed bytes (both member starts; end <= 0: to the end of the file). */
int pc_gz_member_start(const char *path, int64_t pos, int64_t *member_start);
int pc_gzstream_open_range(const char *path, int64_t begin, int64_t end, pc_gzstream **out);
int pc_gzstream_next(pc_gzstream *s, int64_t target_bytes, int64_t min_reads, pc_readset **out, int *eof);
void pc_gzstream_close(pc_gzstream *s);

#ifdef __cplusplus
}
#endif
#endif /* PORECHOP_AMD_H */
