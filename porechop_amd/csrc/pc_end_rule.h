// pc_end_rule.h -- can an end-window alignment trim its read at all?  Answered from its score record alone.
//
// Phase B keeps, per read and side, the MAXIMUM trim over the alignments that qualify (nanopore_read.py:166-208):
//   start window:  identity > end_threshold,  read_end != end_size,  read_end - read_start >= min_trim_size  -> read_end + extra
//   end window:    identity > end_threshold,  read_start != 0,       read_end - read_start >= min_trim_size  -> end_size - read_start + extra
// A score-only pass gives every pair's score S and end cell (I adapter bases and Jc window columns consumed) -- the cell the
// traceback starts from.  From those alone (the derivations stand above Pipeline._phase_b_bounds, whose integer arithmetic
// this header keeps):
//   start window:  read_end = Jc, so none if Jc + 1 < min_trim_size, none if Jc == n == end_size (the path ends in the last
//                  column of a full window); else trim <= Jc + 1 + extra
//   end window:    a qualifying path starts on the first row at a column j0 >= 1, consumes all I adapter bases and b = Jc - j0
//                  window columns with  bmin = ceil((S + g I) / (match + g)) <= b <= bmax = I + max(0, match I - S) / g,
//                  g = min(|open|, |extend|): none if Jc - 1 < bmin or bmax + 1 < min_trim_size; else
//                  trim <= end_size - max(1, Jc - bmax) + extra
//   either side:   identity > end_threshold over at least min(I, Jc) columns needs  S > floor(c max(1, min(I, Jc))),
//                  c = tau match - (1 - tau) P,  tau = (end_threshold - 1e-6) / 100,  P = the dearest non-matching column
//                  (no such bound when c <= 0)
// A pair whose bound is not above 0 cannot raise a trim from 0: it need not be traced, and "no alignment" is the same answer.
// This is ONE round -- no comparison with the trims other pairs have reached, nothing about barcode calls.  Anything that is
// not a plain score record (flag -2) is traced.
//
// Plain C++17 for the host and the device: no runtime include, usable from the kernels between the two passes and from
// tests/host/test_end_rule.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCR_HD __host__ __device__
#else
#define PCR_HD
#endif

namespace pcr {

// What the caller sets for a scan (pc_end_rule of the C interface) with the context's scores: one per call.
struct EndRule {
    int32_t match = 3, mismatch = -6, gap_open = -5, gap_extend = -2;
    int32_t end_size = 150, min_trim_size = 4, extra_end_trim = 2;
    double ident_c = 0.0;          // c above; <= 0: the scheme gives no identity bound
};

inline EndRule make_end_rule(int match, int mismatch, int gap_open, int gap_extend, int end_size, int min_trim_size,
                             int extra_end_trim, double end_threshold)
{
    EndRule r;
    r.match = match; r.mismatch = mismatch; r.gap_open = gap_open; r.gap_extend = gap_extend;
    r.end_size = end_size; r.min_trim_size = min_trim_size; r.extra_end_trim = extra_end_trim;
    const double tau = (end_threshold - 1e-6) / 100.0;
    int P = 0;
    if (-mismatch > P) P = -mismatch;
    if (-gap_open > P) P = -gap_open;
    if (-gap_extend > P) P = -gap_extend;
    // (two roundings, as the float64 expression of the torch code: never contracted into one)
    const volatile double earned = tau * (double)match, lost = (1.0 - tau) * (double)P;
    r.ident_c = earned - lost;
    return r;
}

PCR_HD inline int64_t floor_div(int64_t a, int64_t b)      // b > 0
{
    int64_t q = a / b;
    if ((a % b) != 0 && a < 0) --q;
    return q;
}

// Upper bound on the trim the pair can contribute; <= 0: none.  side 0: a start window, 1: an end window; n: the window's
// length, m: the adapter's.  flag, Jc, I, S: fields 0, 1, 2 and 4 of the score record.
PCR_HD inline int64_t trim_bound(const EndRule &r, int side, int flag, int S, int I, int Jc, int n, int m)
{
    const int64_t kTrace = (int64_t)1 << 20;
    if (flag != -2 || I < 0 || Jc < 0 || I > m || Jc > n) return kTrace;     // not a plain score record of this pair: trace it
    int64_t ub;
    if (side == 0) {
        const bool ok_s = ((int64_t)Jc + 1 >= r.min_trim_size) && !(Jc == n && n == r.end_size);
        ub = ok_s ? (int64_t)Jc + 1 + r.extra_end_trim : 0;
    } else {
        const int64_t g = -r.gap_open < -r.gap_extend ? -(int64_t)r.gap_open : -(int64_t)r.gap_extend;
        if (g > 0 && r.match + g > 0) {
            const int64_t bmin = floor_div((int64_t)S + g * I + (r.match + g - 1), r.match + g);
            const int64_t over = (int64_t)r.match * I - S;
            const int64_t bmax = I + (over > 0 ? over : 0) / g;
            const bool ok_e = ((int64_t)Jc - 1 >= bmin) && (bmax + 1 >= r.min_trim_size);
            const int64_t back = Jc - bmax > 1 ? Jc - bmax : 1;
            ub = ok_e ? (int64_t)r.end_size - back + r.extra_end_trim : 0;
        } else {
            ub = (int64_t)r.end_size - 1 + r.extra_end_trim;                 // (a scheme the derivation does not cover: no bound)
        }
    }
    if (r.ident_c > 0.0) {
        const int mn = I < Jc ? I : Jc;
        const double need_f = r.ident_c * (double)(mn > 1 ? mn : 1);
        int64_t need = (int64_t)need_f;                                      // floor of a non-negative product
        if ((double)need > need_f) --need;
        if (!((int64_t)S > need)) ub = 0;
    }
    return ub;
}

PCR_HD inline bool can_trim(const EndRule &r, int side, int flag, int S, int I, int Jc, int n, int m)
{
    return trim_bound(r, side, flag, S, I, Jc, n, m) > 0;
}

}  // namespace pcr
