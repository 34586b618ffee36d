"""Plain host reference of the per-read glue kernels (TEST INFRASTRUCTURE; no torch, no GPU).

Per read, line by line, what porechop/nanopore_read.py decides from the alignments' 7-field strings:
  record_fields        align_adapter              nanopore_read.py:476-491   (format, then parse: no rounding here)
  end_trims            find_start_trim / _end     nanopore_read.py:166-208   (ref_pipeline.phase_b's rule)
  barcode_call         determine_barcode          nanopore_read.py:399-466   (ref_pipeline.determine_barcode)
  trimmed_interval     seq[start : len - end]     nanopore_read.py:56-62     (Python slice arithmetic)
  middle_hit           full_score >= threshold    nanopore_read.py:218-226
  consume              one round of find_middle_adapters for one read (nanopore_read.py:210-243)
  select_bound / select_round   which end-window pairs the exact pruning of phase B has traced (the rules of
                       porechop_amd/pipeline.py, "Exact pruning of phase B", per read in plain Python)

Records are the library's int32[8]: rs, re, as, ae, score, matches, aligned_len, full_len.  Field 0 == -1 is a failed
alignment.  In phase B a record with field 0 == -2 is a score record the exact pruning left untraced (pc_select.hip); it
reads as "no alignment" there, like -1.
"""
import math

from porechop_amd.batch import format_results
from tests.ref_pipeline import determine_barcode

STAT_BIG = 1 << 40


class Fields:
    """(full, partial, read_start, read_end) of many records, through the reference's own strings.  The strings depend
    on (matches, aligned_len, full_len) only, so every distinct triple is formatted once."""

    def __init__(self):
        self._memo = {}

    def identities(self, triples):
        todo = [t for t in dict.fromkeys(triples) if t not in self._memo]
        if todo:
            recs = [[0, 0, 0, 0, 0, m, al, fl] for m, al, fl in todo]
            for t, s in zip(todo, format_results(recs)):
                parts = s.split(",")
                self._memo[t] = (float(parts[6]), float(parts[5]))
        return [self._memo[t] for t in triples]

    def of(self, recs, score_only_fails=False):
        """-> list of (full, partial, read_start, read_end), as ref_pipeline.align_adapter returns them."""
        recs = [tuple(int(x) for x in r) for r in recs]
        ids = self.identities([(r[5], r[6], r[7]) for r in recs])
        out = []
        for r, (full, partial) in zip(recs, ids):
            if r[0] == -1 or (score_only_fails and r[0] == -2):
                out.append((0.0, 0.0, -1, 0))
            else:
                out.append((full, partial, r[0], r[1] + 1))
        return out


_FIELDS = Fields()


def record_fields(recs, score_only_fails=False):
    return _FIELDS.of(recs, score_only_fails)


def identity(matches, length):
    """The full identity the reference parses back from a record with these fields."""
    return _FIELDS.identities([(matches, length, length)])[0][0]


def end_trims(fields, sides, end_size, min_trim_size, extra_end_trim, end_threshold):
    """One read: fields[j] = (full, partial, rs, re) of job j, or None where the job is not traced for this read.
    -> (start_trim, end_trim) by ref_pipeline.phase_b's rule."""
    start_trim = end_trim = 0
    for f, side in zip(fields, sides):
        if f is None:
            continue
        full, partial, rs, re = f
        if side == 0:
            if partial > end_threshold and re != end_size and re - rs >= min_trim_size:
                start_trim = max(start_trim, re + extra_end_trim)
        else:
            if partial > end_threshold and rs != 0 and re - rs >= min_trim_size:
                end_trim = max(end_trim, (end_size - rs) + extra_end_trim)
    return start_trim, end_trim


def barcode_call(fields, bins, barcode_threshold, barcode_diff, require_two):
    """One read: bins = [(start job or -1, end job or -1)] in the order the reference inserts the names.  A missing job
    (-1) or an untraced one (fields[j] is None) is left out of the reference's dicts.  -> bin index, or -1 for 'none'."""
    start_scores, end_scores = {}, {}
    for k, (sj, ej) in enumerate(bins):
        if sj >= 0 and fields[sj] is not None:
            start_scores[k] = fields[sj][0]
        if ej >= 0 and fields[ej] is not None:
            end_scores[k] = fields[ej][0]
    name = determine_barcode(start_scores, end_scores, barcode_threshold, barcode_diff, require_two)
    return -1 if name == "none" else name


def trimmed_interval(length, start_trim, end_trim):
    """-> (start, length) of seq[start_trim : len(seq) - end_trim] (the whole read when both trims are 0)."""
    if not start_trim and not end_trim:
        return 0, length
    r = range(length)[start_trim:length - end_trim]
    return r.start, len(r)


def trim_stats(lengths):
    """[reads with a non-empty interval, longest, STAT_BIG - shortest non-empty (0: none), sum of lengths]"""
    live = [t for t in lengths if t > 0]
    return [len(live), max(lengths, default=0), STAT_BIG - min(live) if live else 0, sum(lengths)]


def middle_hit(field, threshold):
    """(full, hit) of one whole-read alignment: full_score >= middle_threshold."""
    full = field[0]
    return full, full >= threshold


def consume(fulls, rs, re, cur, threshold):
    """One consuming round of find_middle_adapters for one read standing at adapter `cur`: fulls[a] / rs[a] / re[a] are
    adapter a's full identity, read_start and read_end (rs == -1: failed, full_score 0.0).
    -> (adapter that hits or None, bases to mask, alignments consumed)"""
    A = len(fulls)
    for a in range(cur, A):
        full = 0.0 if rs[a] == -1 else fulls[a]
        if full >= threshold:
            return a, max(0, re[a] - rs[a]), a - cur + 1
    return None, 0, A - cur


def select_bound(rec, side, m, nwin, end_size, min_trim_size, extra_end_trim, end_threshold, scores):
    """Upper bounds on what the alignment behind one score record (-2, Jc, I, 0, S, ...) can contribute: (largest trim, largest
    full identity, S).  side 0: a start window; nwin: the window's length; m: the adapter's."""
    match, mismatch, gap_open, gap_extend = scores
    flag, Jc, I, S = int(rec[0]), int(rec[1]), int(rec[2]), int(rec[4])
    if flag != -2:                                       # not a plain score record: always traced
        return 1 << 20, 100.0, S
    mn = min(I, Jc)
    ub_full = 100.0 * min(mn, m) / m
    if side == 0:
        # the trim is the end column + 1 + extra; none below min_trim_size, none for a path that ends in the last column of a full window
        ok = Jc + 1 >= min_trim_size and not (Jc == nwin and nwin == end_size)
        ub = Jc + 1 + extra_end_trim if ok else 0
    else:
        g = min(-gap_open, -gap_extend)
        if g > 0 and match + g > 0:
            bmin = -((-(S + g * I)) // (match + g))       # fewest columns a path of score S over I adapter bases spans
            bmax = I + max(0, match * I - S) // g        # most
            ok = Jc - 1 >= bmin and bmax + 1 >= min_trim_size
            ub = end_size - max(1, Jc - bmax) + extra_end_trim if ok else 0
        else:
            ub = end_size - 1 + extra_end_trim
    pen = max(-mismatch, -gap_open, -gap_extend, 0)
    tau = (end_threshold - 1e-6) / 100.0
    c = tau * match - (1.0 - tau) * pen                   # a trim needs S > c min(I, Jc)
    if c > 0.0 and not S > math.floor(c * max(mn, 1)):
        ub = 0
    return ub, ub_full, S


def select_round(recs, offs, sides, lens, calls, start_len, end_len, n, params, scores, rnd, call_level, call_level_diff,
                 prev=None, so_far=None, best_full=None):
    """One round of the selection for n reads: recs[offs[j] + r] is job j's score record of read r; params = (end_size,
    min_trim_size, extra_end_trim, end_threshold).  Round 1: per read and side the two best-scoring pairs that can trim
    and the two best-scoring barcode pairs (calls[j]), earlier job first among equal scores.  Round 2 (prev: the bits of
    round 1, so_far: (start_trim, end_trim) per read, best_full[side][r]): what can still beat the trims so far or come
    within call_level_diff of the best barcode identity.  -> (bits[j][r], ub_trim[j][r], ub_full[j][r])"""
    match, mismatch, gap_open, gap_extend = scores
    pen = max(-mismatch, -gap_open, -gap_extend, 0)
    J = len(sides)
    calls_on = call_level < 1e8
    bits = [[False] * n for _ in range(J)]
    ub_t = [[0] * n for _ in range(J)]
    ub_f = [[0.0] * n for _ in range(J)]
    for r in range(n):
        b = [select_bound(recs[offs[j] + r], sides[j], lens[j], end_len[r] if sides[j] else start_len[r], *params, scores) for j in range(J)]
        for j in range(J):
            ub_t[j][r], ub_f[j][r] = b[j][0], b[j][1]
        if rnd == 1:
            for side in (0, 1):
                for want_call in (False, True):
                    if want_call and not calls_on:
                        continue
                    cand = [(-b[j][2], j) for j in range(J) if sides[j] == side and b[j][2] >= 0 and
                            ((calls[j] != 0) if want_call else (b[j][0] > 0))]
                    for _, j in sorted(cand)[:2]:
                        bits[j][r] = True
        else:
            for j in range(J):
                if prev[j][r]:
                    continue
                side, m = sides[j], lens[j]
                pick = b[j][0] > so_far[side][r]
                if calls_on and calls[j]:
                    lvl = max(best_full[side][r], call_level + call_level_diff) - call_level_diff - 1e-6
                    smin = math.floor(m * ((lvl / 100.0) * (match + pen) - pen) - 1e-9)
                    pick = pick or (b[j][1] >= lvl and b[j][2] >= smin)
                bits[j][r] = pick
    return bits, ub_t, ub_f
