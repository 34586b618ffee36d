// pc_explain.hip -- WHY a read was trimmed and called: the per-read data behind pc_phase_b_reduce's two trims and bin.
//
// The reference keeps, per read, the end alignments that qualified for a trim (start_adapter_alignments /
// end_adapter_alignments, nanopore_read.py:178-183,200-205) and the best and second-best barcode of each side
// (nanopore_read.py:399-416).  pc_reduce.hip folds the same records into two trims and a call; this kernel reads them
// once more and keeps the reasons.  Same inputs, same conventions: record layout, job order, side, absent bins (-1),
// untraced pairs (mask bit clear), -1 / -2 records = "no alignment", identities as the %f-rounded doubles.
//
// Two passes of ONE kernel, because the number of qualifying alignments is not known in advance:
//   summary (hit_first == NULL)  12 ints + 4 doubles per read: trims, counts, deciding jobs, best / second-best bins
//   fill    (hit_first given)    the qualifying alignments themselves, read r's rows from hit_first[r]: start
//                                alignments in job order, then end alignments in job order (the reference's append order)
// HBM-bound integer work shaped like reduce_kernel: one thread per read, adjacent threads on adjacent 32-byte records
// (written as two 16-byte loads each, which the compiler narrows to the live fields -- an 8-byte and a 12-byte load: the same
// 32-byte sectors, coalesced per job), a wave's 64 reads share one mask word per job.  The barcode entries are
// picked up in the same walk over the jobs (job -> bin tables, inverted on the host), so every record is loaded once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pc_kernels.h"
#include "pc_record.h"

namespace pck {

namespace {

// The first two entries of Python's stable descending sort of one side's (bin, score) entries: the order is score
// descending, then bin ascending (among equal scores the entry inserted first wins), so the two can be kept while the
// entries arrive in ANY order.  v = -1: no entry yet (identities are >= 0).
struct Top2 {
    int b0 = -1, b1 = -1;
    double v0 = -1.0, v1 = -1.0;
    __device__ __forceinline__ void offer(int k, double v)
    {
        if (v > v0 || (v == v0 && k < b0)) { v1 = v0; b1 = b0; v0 = v; b0 = k; }
        else if (v > v1 || (v == v1 && k < b1)) { v1 = v; b1 = k; }
    }
};

}  // namespace

__global__ __launch_bounds__(256) void explain_kernel(ExplainArgs a)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const bool fill = a.hit_first != nullptr;
    auto untraced = [&](int j) -> bool {
        return a.traced_mask && !((a.traced_mask[(int64_t)j * a.mask_words + (r >> 6)] >> (r & 63)) & 1ull);
    };
    // fill pass: the read's rows are [hit_first[r], hit_first[r + 1]); the end alignments follow the start alignments
    int64_t s_row = 0, e_row = 0, row_end = 0;
    if (fill) {
        s_row = a.hit_first[r];
        row_end = a.hit_first[r + 1];
        e_row = s_row + a.summary[r * EXPLAIN_INTS + 2];
    }
    auto put = [&](int64_t row, int j, const Rec &rec) {
        if (row >= row_end) return;                     // a prefix sum that does not match the summary writes nothing
        int2 *o = (int2 *)(a.hits + row * EXPLAIN_HIT_INTS);
        o[0] = int2{j, rec.rs};
        o[1] = int2{rec.re + 1, rec.matches};
        o[2] = int2{rec.aligned_len, rec.full_len};
    };
    const bool bins_inline = !fill && a.nbins > 0 && a.job_sbin;
    Top2 S, E;
    int start_trim = 0, end_trim = 0, ns = 0, ne = 0, sj = -1, ej = -1;
    for (int j = 0; j < a.njobs; ++j) {
        if (untraced(j)) continue;
        const Rec rec = load_rec(a.records, a.job_off[j] + r);
        if (bins_inline) {
            const int sb = a.job_sbin[j], eb = a.job_ebin[j];
            if (sb >= 0 || eb >= 0) {
                const double full = full_identity(rec);
                if (sb >= 0) S.offer(sb, full);
                if (eb >= 0) E.offer(eb, full);
            }
        }
        if (rec.rs < 0) continue;                      // -1: no alignment; -2: a score record left untraced (pc_select.hip)
        const double partial = identity(rec.matches, rec.aligned_len);
        const int rs = rec.rs, re = rec.re + 1;
        if (!(partial > a.end_threshold) || re - rs < a.min_trim_size) continue;
        if (a.job_side[j] == 0) {
            if (re == a.end_size) continue;
            ++ns;
            const int t = re + a.extra_end_trim;
            if (t > start_trim) { start_trim = t; sj = j; }       // strict: the FIRST job that reaches the maximum
            if (fill) put(s_row++, j, rec);
        } else {
            if (rs == 0) continue;
            ++ne;
            const int t = (a.end_size - rs) + a.extra_end_trim;
            if (t > end_trim) { end_trim = t; ej = j; }
            if (fill) put(e_row++, j, rec);
        }
    }
    if (fill) return;
    if (a.nbins > 0 && !a.job_sbin) {
        // a job that serves several bins of one side has no single inverse entry: walk the bins instead (a second load
        // of their records, as reduce_kernel does)
        auto walk = [&](const int32_t *jobs, Top2 &t) {
            for (int k = 0; k < a.nbins; ++k) {
                const int j = jobs[k];
                if (j < 0 || untraced(j)) continue;
                t.offer(k, full_identity(load_rec(a.records, a.job_off[j] + r)));
            }
        };
        walk(a.bin_start, S);
        walk(a.bin_end, E);
    }
    int4 *o = (int4 *)(a.summary + r * EXPLAIN_INTS);
    o[0] = int4{start_trim, end_trim, ns, ne};
    o[1] = int4{sj, ej, S.b0, S.b1};
    o[2] = int4{E.b0, E.b1, 0, 0};
    double2 *d = (double2 *)(a.bscore + r * 4);
    d[0] = double2{S.b0 >= 0 ? S.v0 : 0.0, S.b1 >= 0 ? S.v1 : 0.0};
    d[1] = double2{E.b0 >= 0 ? E.v0 : 0.0, E.b1 >= 0 ? E.v1 : 0.0};
}

int launch_explain(const ExplainArgs &a, void *stream)
{
    if (a.n <= 0) return 0;
    const unsigned grid = (unsigned)((a.n + 255) / 256);
    hipLaunchKernelGGL(explain_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace pck
