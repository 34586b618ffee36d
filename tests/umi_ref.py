"""TEST INFRASTRUCTURE: the UMI rule of DESIGN.md section 16 restated in plain Python over tests/wild_ref.py's paths
(read_first, adapter_first, forward cigar) and letter sets.  It shares no code with porechop_amd/csrc/pc_umi.h and binds to
nothing under test.

    span(adapter)                       -> (u0, u1) or None
    extract(path, (u0, u1))             -> (first, length, covered, complete)
    qualifies(record, side, rule)       -> bool          rule = (end_size, min_trim_size, extra_end_trim, end_threshold)
    umi_many(windows, adapter, ...)     -> (records int32 [n, 8], umi int32 [n, 4] = status, first, length, covered)
"""
import numpy as np

from tests import wild_ref


def span(adapter, wildcards=True):
    """Rows (0-based, inclusive) from the first to the last letter that stands for two or more bases."""
    adapter = adapter if isinstance(adapter, (bytes, bytearray)) else adapter.encode()
    rows = [k for k, b in enumerate(adapter) if bin(wild_ref.letter_set(b, wildcards) & 15).count("1") >= 2]
    return (rows[0], rows[-1]) if rows else None


def extract(path, sp):
    """Every consumed window column with the adapter row it was consumed against (a diagonal step) or before (an
    insertion); the UMI's columns picked from that list."""
    read_first, adapter_first, cigar = path
    u0, u1 = sp
    i, j = read_first, adapter_first
    diagonal, inserted, rows = [], [], []          # (column, row) pairs; rows the path consumes
    for op in wild_ref.expand(cigar):
        if op in "=X":
            diagonal.append((i, j))
            rows.append(j)
            i += 1
            j += 1
        elif op == "I":
            inserted.append((i, j))
            i += 1
        else:
            rows.append(j)
            j += 1
    under = sorted([c for c, r in diagonal if u0 <= r <= u1] + [c for c, r in inserted if u0 < r <= u1])
    covered = sum(1 for c, r in diagonal if u0 <= r <= u1)
    complete = adapter_first <= u0 and bool(rows) and rows[-1] >= u1
    if not under:
        return -1, 0, covered, complete
    assert under == list(range(under[0], under[0] + len(under))), under       # one run
    return under[0], len(under), covered, complete


def identity(matches, length):
    """The double Python sees: the reference's "%f", parsed back."""
    return float("%f" % (100.0 * matches / length)) if length else float("nan")


def qualifies(rec, side, rule):
    """nanopore_read.py:166-208: may this end-window alignment trim its read at all?"""
    end_size, min_trim_size, _extra, end_threshold = rule
    rs, re_ = int(rec[0]), int(rec[1]) + 1
    if rs < 0:
        return False
    if not identity(int(rec[5]), int(rec[6])) > end_threshold:
        return False
    if re_ - rs < min_trim_size:
        return False
    return re_ != end_size if side == 0 else rs != 0


def classify(rec, path, sp, side=0, rule=None):
    """-> (status, first, length, covered)"""
    if int(rec[0]) < 0:
        return 1, -1, 0, 0
    if rule is not None and not qualifies(rec, side, rule):
        return 2, -1, 0, 0
    first, length, covered, complete = extract(path, sp)
    return (0 if complete else 3), first, length, covered


def umi_many(windows, adapter, scores=(3, -6, -5, -2), side=0, rule=None):
    sp = span(adapter)
    assert sp is not None, "the adapter has no span"
    recs, paths = wild_ref.align_many([(w, adapter) for w in windows], scores, wildcards=True)
    umi = np.zeros((len(windows), 4), dtype=np.int32)
    for k in range(len(windows)):
        umi[k] = classify(recs[k], paths[k], sp, side, rule)
    return recs, umi
