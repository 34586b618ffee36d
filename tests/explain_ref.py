"""Plain host restatement of pc_phase_b_explain's contract (TEST INFRASTRUCTURE; numpy for the arrays, no torch, no GPU).

Per read, line by line, what porechop/nanopore_read.py keeps about its end alignments:
  qualifying alignments   find_start_trim / find_end_trim   nanopore_read.py:166-208  (the tuples it appends, in its order)
  best / second best      determine_barcode                 nanopore_read.py:399-416  (Python's own stable sort)
from the library's int32[8] records through the reference's own strings (tests/glue_ref.record_fields).  A record with
field 0 == -1 or -2 is "no alignment"; a bin entry without a job (-1) or whose pair is not traced is left out of the dicts.
tests/test_explain_host_model.py checks this model against tests/ref_pipeline.py on oracle-driven records."""
import numpy as np

from tests.glue_ref import record_fields

EXPLAIN_INTS = 12


def explain(records, n, job_off, sides, end_size, min_trim_size, extra_end_trim, end_threshold, bins=(), traced=None):
    """records int [*, 8]; job j's record of read r at records[job_off[j] + r]; traced: bool [J, n] or None (all traced).
    bins: [(start job or -1, end job or -1)] -> (summary int32 [n, 12], bscore float64 [n, 4], hit_first int64 [n + 1],
    hits int32 [total, 6])."""
    records = np.asarray(records)
    J = len(sides)
    fields = [record_fields(records[job_off[j]:job_off[j] + n], score_only_fails=True) for j in range(J)]
    present = lambda j, r: traced is None or bool(traced[j][r])
    summary = np.zeros((n, EXPLAIN_INTS), dtype=np.int32)
    bscore = np.zeros((n, 4), dtype=np.float64)
    rows, hit_first = [], np.zeros(n + 1, dtype=np.int64)
    for r in range(n):
        lists = ([], [])                                   # the reference's two lists, in append order
        trim, decided = [0, 0], [-1, -1]
        for j in range(J):
            if not present(j, r):
                continue
            full, partial, rs, re = fields[j][r]
            if rs < 0:
                continue
            side = 1 if sides[j] else 0
            if side == 0:
                ok = partial > end_threshold and re != end_size and re - rs >= min_trim_size
                amount = re + extra_end_trim
            else:
                ok = partial > end_threshold and rs != 0 and re - rs >= min_trim_size
                amount = (end_size - rs) + extra_end_trim
            if ok:
                if amount > trim[side]:                    # max(): the first job that reaches the final value decides
                    trim[side], decided[side] = amount, j
                rec = records[job_off[j] + r]
                lists[side].append([j, rs, re, int(rec[5]), int(rec[6]), int(rec[7])])
        summary[r, 0:2] = trim
        summary[r, 2:4] = [len(lists[0]), len(lists[1])]
        summary[r, 4:6] = decided
        rows += lists[0] + lists[1]
        hit_first[r + 1] = len(rows)
        for col, which in ((0, 0), (1, 1)):
            scores = {}
            for k, b in enumerate(bins):
                j = b[which]
                if j >= 0 and present(j, r):
                    scores[k] = fields[j][r][0]
            ranked = sorted(scores.items(), reverse=True, key=lambda x: x[1])     # nanopore_read.py:404-407
            for rank in range(2):
                k, v = ranked[rank] if len(ranked) > rank else (-1, 0.0)
                summary[r, 6 + 2 * col + rank] = k
                bscore[r, 2 * col + rank] = v
    hits = np.array(rows, dtype=np.int32).reshape(-1, 6)
    return summary, bscore, hit_first, hits


def implied_call(summary_row, bscore_row, barcode_threshold, barcode_diff, require_two):
    """The barcode call (bin index or -1) that follows from one read's best / second-best bins and scores
    (nanopore_read.py:418-466): what pc_phase_b_reduce must give on the same records."""
    sb, s2, eb, e2 = (int(x) for x in summary_row[6:10])
    sv, s2v, ev, e2v = (float(x) for x in bscore_row)
    if require_two:
        ok = sv >= barcode_threshold and ev >= barcode_threshold and sv >= s2v + barcode_diff and ev >= e2v + barcode_diff and sb == eb
        return sb if ok else -1
    # the merged list of the reference: stable descending sort of start entries then end entries, each name once
    merged = sorted([(k, v) for k, v in ((sb, sv), (s2, s2v)) if k >= 0] + [(k, v) for k, v in ((eb, ev), (e2, e2v)) if k >= 0],
                    reverse=True, key=lambda x: x[1])
    best = merged[0] if merged else (-1, 0.0)
    others = [x for x in merged if x[0] != best[0]]
    second = others[0] if others else (-1, 0.0)
    return best[0] if best[1] >= barcode_threshold and best[1] >= second[1] + barcode_diff else -1
