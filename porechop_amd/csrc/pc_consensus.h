// pc_consensus.h -- the rule of the UMI consensus: one sequence per group of reads, by a column vote over banded alignments.
//
// CODES.  A C G T = 0 .. 3, U as T, either letter case; any other byte is code 4, which matches nothing and casts no vote.
//
// ALIGNMENT of a member b (lb >= 0 bases) to the template a (la >= 1 bases): the global unit-cost edit distance inside a band
// around the stretched diagonal.  Cell (i, j), 0 <= i <= la, 0 <= j <= lb, is inside iff |j - floor(i * lb / la)| <= band (the
// product in 64 bits); a cell outside is INF.  (0, 0) and (la, lb) are always inside.  Two rows of the band touch as long as
// their centres lie at most 2 band + 1 apart, i.e. for lb up to about (2 band + 1) la; beyond that no path stays inside, the
// distance is INF and the member is rejected like any member that is too far.
//     D[0][j] = j,  D[i][j] = min(D[i-1][j-1] + (code a[i-1] == code b[j-1] < 4 ? 0 : 1), D[i-1][j] + 1, D[i][j-1] + 1)
// A member is REJECTED iff d * 100 > max_err_pct * max(la, lb), d = D[la][lb], in 64 bits.
//
// TRACEBACK ORDER (stated here, once).  From (la, lb); at each cell the DIAGONAL when it reproduces the cell's value,
// otherwise the step that consumes a TEMPLATE COLUMN (a deletion in the member: from (i-1, j)), otherwise the step that
// consumes a MEMBER BASE (an insertion: from (i, j-1)).  In row 0 only insertions are left, in column 0 only deletions.
//
// TRACE.  Two bits per band cell (OP_DIAG / OP_DEL / OP_INS), rows 1 .. la, cell k = j - (floor(i * lb / la) - band) of a row,
// 0 <= k < W = 2 band + 1 <= 255.  A row is 64 bytes: byte k / CPL holds cell k at bits 2 (k % CPL), CPL = ceil(W / 64) -- on
// the device byte t of a row is lane t's, so a wave stores a row as one line of 64 bytes.
//
// VOTES of one group, uint32 counters: column i has five (A C G T deletion) at 5 i + c; gap g (before column g, 0 <= g <= la)
// has INS_SLOTS slots of four at 5 la + (g * INS_SLOTS + s) * 4 + c: votes_per_group(la) = 21 la + 16 in all.  A diagonal step
// votes for the member's base in its column, a deletion for the column's fifth counter, and a member with k inserted bases in
// gap g votes for its s-th inserted base in slot s for s < min(k, INS_SLOTS).  The template votes for its own base in every
// column.
//
// CALL.  Column i emits the leader of its five counters, nothing when deletion leads; ties go to the template's own base
// when it is among the leaders, otherwise to the smallest of A < C < G < T < deletion.  Slot (g, s) is emitted iff twice the
// sum of its four counters exceeds `voters`; its base is its leader, ties to the smallest code.  Output order: gap 0's slots,
// column 0, gap 1's slots, ..., gap la's slots: at most 5 la + 4 bytes.
//
// QUALITY (only when the caller hands in a table of 256 Phred values).  An emitted base gets qtab[min(margin, 255)], margin its
// votes less those of its strongest alternative: column_margin() and slot_margin() below state it, in integers.
//
// STRAND.  A member of strand 1 is read as its REVERSE COMPLEMENT: its base j (0-based) is the complement of the stored byte
// lb - 1 - j -- on codes 0 <-> 3, 1 <-> 2, code 4 stays 4 (comp_code); U reads as T, whose complement is A.  member_byte() is the
// one place that says so: the device's two refills of a member's bytes go through it, and everything downstream (DP, trace,
// walk, votes, call) sees a member of strand 1 exactly as it would see the materialised reverse complement.  Templates are
// never flipped.
//
// Plain C++ for the host and the device: no runtime include.  fill() is the serial form of the DP (the device sweeps a row
// with its wave and a min-plus prefix scan: the same values, hence the same trace); walk(), the call rule and the layouts
// are the device's own code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCC_HD __host__ __device__ inline
#define PCC_HD_MEMBER __host__ __device__
#else
#define PCC_HD inline
#define PCC_HD_MEMBER
#endif

#define PCC_INS_SLOTS 4

namespace pcc {

constexpr int INS_SLOTS = PCC_INS_SLOTS;
constexpr int MAX_BAND = 127;                     // W = 2 band + 1 <= 255 cells: at most four to a lane
constexpr int MAX_LEN_LIMIT = 1 << 24;            // max_len may not exceed this: d * 100 and 21 la + 16 stay far inside 32 / 64 bits
constexpr int32_t INF = 0x3fffffff;
constexpr int OP_DIAG = 0, OP_DEL = 1, OP_INS = 2;
constexpr int ST_ACCEPTED = 0, ST_REJECTED = 1, ST_INVALID = 2;
constexpr int TRACE_ROW_BYTES = 64;

PCC_HD int code(uint8_t ch)
{
    switch (ch | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': case 'u': return 3;
    default: return 4;
    }
}

// the code of the complementary base: A <-> T, C <-> G; code 4 stays 4
PCC_HD int comp_code(int c) { return c < 4 ? 3 - c : 4; }
// a letter whose code is comp_code(code(ch)): what a member of strand 1 shows where its stored byte is ch ('N' for code 4)
PCC_HD uint8_t comp_letter(uint8_t ch)
{
    switch (ch | 0x20) {
    case 'a': return 'T';
    case 'c': return 'G';
    case 'g': return 'C';
    case 't': case 'u': return 'A';
    default: return 'N';
    }
}

// byte `at` (0 <= at < lb) of a member stored at mb as its strand shows it: the stored byte, or for strand 1 the letter of the
// complement of the stored byte lb - 1 - at
PCC_HD uint8_t member_byte(const uint8_t *mb, int64_t lb, int64_t at, bool reverse)
{
    const uint8_t b = mb[reverse ? lb - 1 - at : at];              // one load either way: no branch around it
    return reverse ? comp_letter(b) : b;
}

PCC_HD int width(int band) { return 2 * band + 1; }
PCC_HD int cells_per_lane(int band) { return (width(band) + 63) / 64; }
// the first column of row i's band (may be negative)
PCC_HD int64_t row_lo(int64_t i, int64_t la, int64_t lb, int band) { return i * lb / la - band; }
PCC_HD bool rejected(int64_t d, int64_t la, int64_t lb, int max_err_pct) { return d * 100 > (int64_t)max_err_pct * (la > lb ? la : lb); }

PCC_HD int64_t votes_per_group(int64_t la) { return 21 * la + 4 * INS_SLOTS; }
PCC_HD int64_t col_counter(int64_t i, int c) { return 5 * i + c; }
PCC_HD int64_t slot_counter(int64_t la, int64_t g, int s, int c) { return 5 * la + (g * INS_SLOTS + s) * 4 + c; }
PCC_HD int64_t cons_capacity(int64_t la) { return 5 * la + INS_SLOTS; }

// trace bytes of one pair whose template has la columns: rows 0 .. la (row 0 is never written or read)
PCC_HD int64_t trace_bytes(int64_t la) { return (la + 1) * TRACE_ROW_BYTES; }
PCC_HD int64_t trace_byte(int64_t i, int k, int cpl) { return i * TRACE_ROW_BYTES + k / cpl; }
PCC_HD int trace_shift(int k, int cpl) { return 2 * (k % cpl); }

// The serial DP: `row` holds W values, `trace` trace_bytes(la) bytes (rows 1 .. la are written).  -> D[la][lb], INF when no
// path stays inside the band.
PCC_HD int32_t fill(const uint8_t *a, int la, const uint8_t *b, int lb, int band, int32_t *row, uint8_t *trace)
{
    const int W = width(band), cpl = cells_per_lane(band);
    int64_t lo = -band;
    for (int k = 0; k < W; ++k) {
        const int64_t j = lo + k;
        row[k] = (j >= 0 && j <= lb) ? (int32_t)j : INF;
    }
    for (int i = 1; i <= la; ++i) {
        const int64_t lo_new = row_lo(i, la, lb, band), sh = lo_new - lo;
        const int ca = code(a[i - 1]);
        int32_t diag = (sh >= 1 && sh - 1 < W) ? row[sh - 1] : INF, left = INF;
        for (int t = 0; t < TRACE_ROW_BYTES; ++t) trace[(int64_t)i * TRACE_ROW_BYTES + t] = 0;
        for (int k = 0; k < W; ++k) {
            const int64_t j = lo_new + k;
            const int32_t up = (k + sh < W) ? row[k + sh] : INF;
            int32_t v = INF;
            int op = OP_INS;
            if (j >= 0 && j <= lb) {
                int32_t dv = INF;
                if (j >= 1) {
                    const int cb = code(b[j - 1]);
                    dv = diag + ((ca == cb && ca < 4) ? 0 : 1);
                }
                const int32_t uv = up + 1, lv = left + 1;
                v = dv < uv ? dv : uv;
                if (lv < v) v = lv;
                if (v > INF) v = INF;
                op = (dv == v) ? OP_DIAG : (uv == v ? OP_DEL : OP_INS);
            }
            row[k] = v;
            left = v;
            diag = up;
            trace[trace_byte(i, k, cpl)] |= (uint8_t)(op << trace_shift(k, cpl));
        }
        lo = lo_new;
    }
    return row[band];                              // (la, lb): lb - (lb - band)
}

// Readers of a member's bases and of a pair's trace over plain memory; the device has its own, which stage both in LDS.
struct PtrSeq {
    const uint8_t *p;
    PCC_HD_MEMBER uint8_t operator()(int64_t j) const { return p[j]; }
};
struct PtrTrace {
    const uint8_t *p;
    PCC_HD_MEMBER uint8_t operator()(int64_t i, int byte) const { return p[i * TRACE_ROW_BYTES + byte]; }
};

// k / cpl for 0 <= k < 256 and cpl in 1 .. 4 without a division (k * 171 >> 9 == k / 3 up to 255)
PCC_HD int over_cpl(int k, int cpl) { return cpl == 1 ? k : (cpl == 2 ? k >> 1 : (cpl == 4 ? k >> 2 : (k * 171) >> 9)); }

// One trace cell of row i, whose band is centred on `centre` = floor(i lb / la); -1 when column j is outside the band.
// trace(i, t): byte t of row i.
template <class Trace>
PCC_HD int trace_op(Trace &trace, int64_t i, int64_t j, int64_t centre, int band)
{
    const int64_t k = j - (centre - band);
    if (k < 0 || k >= width(band)) return -1;
    const int cpl = cells_per_lane(band), byte = over_cpl((int)k, cpl);
    return (trace(i, byte) >> (2 * ((int)k - byte * cpl))) & 3;
}

// The path of an accepted member from (la, lb) back to (0, 0) and its votes: b(j) is the member's base j, votes(counter)
// adds one to a counter of the member's group.  The walk only ever moves to lower rows and lower bases; the centre of its
// row, floor(i lb / la), is carried down by quotient and remainder (acc = (i lb) mod la): no division per step.  -> false
// when it leaves the band or meets a cell no fill writes (never expected).
template <class Seq, class Trace, class Votes>
PCC_HD bool walk(Seq &b, int la, int lb, int band, Trace &trace, Votes &votes)
{
    const int64_t q = lb / la, r = lb % la;
    int64_t i = la, j = lb, centre = lb, acc = 0;
    while (i > 0 || j > 0) {
        int op = OP_INS;
        if (i > 0) {
            op = j == 0 ? OP_DEL : trace_op(trace, i, j, centre, band);
            if (op < 0 || op > OP_INS) return false;
        }
        if (op == OP_INS) {
            // the run of insertions of gap i ends at base j - 1: find its first base
            int64_t run = 1;
            while (j - run > 0) {
                if (i > 0) {
                    const int o = trace_op(trace, i, j - run, centre, band);
                    if (o < 0 || o > OP_INS) return false;
                    if (o != OP_INS) break;
                }
                ++run;
            }
            for (int s = INS_SLOTS < run ? INS_SLOTS - 1 : (int)run - 1; s >= 0; --s) {       // downwards, as every other read of b
                const int c = code(b(j - run + s));
                if (c < 4) votes(slot_counter(la, i, s, c));
            }
            j -= run;
            continue;
        }
        if (op == OP_DIAG) {
            const int c = code(b(j - 1));
            if (c < 4) votes(col_counter(i - 1, c));
            --j;
        } else {
            votes(col_counter(i - 1, 4));
        }
        --i;
        centre -= q;
        acc -= r;
        if (acc < 0) { acc += la; --centre; }
    }
    return true;
}

// Column call: 0 .. 3 the base emitted, 4 nothing.  v: the five counters, the template's own vote included.
PCC_HD int call_column(const uint32_t *v, int tmpl_code)
{
    uint32_t top = v[0];
    for (int c = 1; c < 5; ++c) top = v[c] > top ? v[c] : top;
    if (tmpl_code < 4 && v[tmpl_code] == top) return tmpl_code;
    for (int c = 0; c < 4; ++c) if (v[c] == top) return c;
    return 4;
}

// Slot call: 0 .. 3 the base emitted, -1 nothing.
PCC_HD int call_slot(const uint32_t *v, uint32_t voters)
{
    const uint64_t sum = (uint64_t)v[0] + v[1] + v[2] + v[3];
    if (2 * sum <= (uint64_t)voters) return -1;
    int best = 0;
    for (int c = 1; c < 4; ++c) if (v[c] > v[best]) best = c;
    return best;
}

PCC_HD uint8_t letter(int c) { return (uint8_t)("ACGT"[c]); }

// QUALITY of an emitted base: qtab[quality_index(margin)], qtab the caller's 256 Phred values (0 .. MAX_QUAL), margin the base's
// VOTE MARGIN -- integers only; no formula is evaluated here, so host and device cannot disagree on a rounding.  A column where
// deletion leads and a slot that is not emitted have no quality.
constexpr int QUAL_ENTRIES = 256;
constexpr int MAX_QUAL = 93;                      // Phred + 33 stays printable
PCC_HD int quality_index(uint32_t margin) { return margin < (uint32_t)QUAL_ENTRIES ? (int)margin : QUAL_ENTRIES - 1; }

// Column whose call is base b < 4.  v: the five counters as the call saw them, the template's own vote included.  The evidence
// e[k] is v[k], less one for the template's code (< 4) when tmpl_counts is 0: an earlier consensus is not a read -- its vote
// still decides ties, but it is no evidence; with tmpl_counts 1 the template is a read of the group and its vote counts.
// margin = max(0, e[b] - max over k != b of e[k]), deletion among the k.
PCC_HD uint32_t column_margin(const uint32_t *v, int tmpl_code, int tmpl_counts, int b)
{
    int64_t lead = 0, rest = 0;
    for (int k = 0; k < 5; ++k) {
        const int64_t e = (int64_t)v[k] - ((tmpl_counts == 0 && k == tmpl_code && tmpl_code < 4) ? 1 : 0);
        if (k == b) lead = e;
        else if (e > rest) rest = e;
    }
    return lead > rest ? (uint32_t)(lead - rest) : 0u;
}

// Slot emitted with base b.  v: the slot's four counters; absent = voters - their sum, the voters that hold no base here (never
// negative: only accepted members vote in slots, at most once each).  margin = max(0, v[b] - max(absent, max over k != b of v[k])).
PCC_HD uint32_t slot_margin(const uint32_t *v, uint32_t voters, int b)
{
    int64_t rest = (int64_t)voters - ((int64_t)v[0] + v[1] + v[2] + v[3]);
    for (int k = 0; k < 4; ++k)
        if (k != b && (int64_t)v[k] > rest) rest = v[k];
    return (int64_t)v[b] > rest ? (uint32_t)((int64_t)v[b] - rest) : 0u;
}

}  // namespace pcc
