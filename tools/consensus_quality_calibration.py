#!/usr/bin/env python3
"""Calibration record of the consensus quality values on the HOST MODEL (porechop_amd.consensus: numpy, no
GPU): seeded groups of 3, 5, 10 and 20 copies of 1 kb originals at 5 % and 10 % errors (a third each of substitutions, insertions
and deletions: tools/consensus_accuracy.py's error model and seeds), two rounds, the default table (vote_err_pct 10, max_qual 60).
Each consensus is aligned to its original with the repository's own banded edit distance and traceback (consensus.align, the
traceback order of csrc/pc_consensus.h); a consensus base is WRONG when it stands against a different base of the original or
against none (an inserted base).  Per quality value that occurs: how many bases carry it, how many of them are wrong, and the
error rate counted beside the one the value claims (10^(-q / 10)); per cell and in total the sum of expected errors against the
errors counted.  Bases of the original the consensus OMITS have no quality and are counted apart.  No threshold is set: a record,
not a gate.  Seeded: the same numbers every time.
   python tools/consensus_quality_calibration.py [trials] [out.txt]      (default 5, profiles/consensus_quality_calibration.txt)"""
import random
import sys
import time
sys.path.insert(0, ".")
import numpy as np
from porechop_amd import consensus as cs

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else "profiles/consensus_quality_calibration.txt"
BAND = 64
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def original(rng, n):                                       # (tools/consensus_accuracy.py's)
    return "".join(rng.choice("ACGT") for _ in range(n))


def copy_of(rng, seq, sub, ins, dele):                      # (tools/consensus_accuracy.py's)
    out = []
    for ch in seq:
        r = rng.random()
        if r < sub:
            out.append(rng.choice([b for b in "ACGT" if b != ch]))
        elif r < sub + dele:
            continue
        else:
            if r < sub + dele + ins:
                out.append(rng.choice("ACGT"))
            out.append(ch)
    return "".join(out).encode()


def as_groups(reads):
    off = np.concatenate([[0], np.cumsum([len(s) + 1 for s in reads])])[:-1].astype(np.int64)
    arena = np.frombuffer(b"".join(s + b"-" for s in reads), dtype=np.uint8)
    return [(1, "K", list(range(len(reads))))], arena, off, np.array([len(s) for s in reads], dtype=np.int64)


def judge(orig, seq):
    """The consensus aligned to its original (the original as the template) -> (per consensus base whether it is wrong, how many
    bases of the original the consensus omits)."""
    a, b = cs.codes(orig), cs.codes(seq)
    la, lb = len(a), len(b)
    d, ops = cs.align(a, b, BAND)
    assert d < cs.INF
    wrong = np.zeros(lb, dtype=bool)
    omitted, i, j = 0, la, lb
    while i > 0 or j > 0:
        op = cs.OP_INS if i == 0 else (cs.OP_DEL if j == 0 else int(ops[i, j - (i * lb // la - BAND)]))
        if op == cs.OP_DIAG:
            wrong[j - 1] = a[i - 1] != b[j - 1]
            i, j = i - 1, j - 1
        elif op == cs.OP_DEL:
            omitted += 1
            i -= 1
        else:
            wrong[j - 1] = True
            j -= 1
    assert int(wrong.sum()) + omitted == d
    return wrong, omitted


t0 = time.time()
table = cs.quality_table()
say("UMI consensus quality values, host model (porechop_amd.consensus), defaults: band %(band)d, rounds %(rounds)d, max_err_pct %(max_err_pct)d" % cs.DEFAULTS +
    "; table: vote_err_pct 10, max_qual 60 (%s ...)" % ", ".join(str(int(q)) for q in table[:6]))
say("originals of 1 kb, %d seeded groups per cell, a third each of substitutions, insertions and deletions" % trials)
say("")
say("1. per cell: expected errors (the sum over the bases of 10^(-q / 10)) against the errors counted")
say("   errors  copies   bases    expected   wrong bases   omitted bases   mean q wrong   mean q right")
by_q = {}
tot_expected = tot_wrong = tot_omitted = tot_bases = 0
for rate in (0.05, 0.10):
    for copies in (3, 5, 10, 20):
        expected, n_wrong, n_omitted, n_bases, q_wrong, q_right = 0.0, 0, 0, 0, [], []
        for trial in range(trials):
            rng = random.Random(1000 * copies + int(rate * 100) * 10 + trial)
            orig = original(rng, 1000)
            reads = [copy_of(rng, orig, rate / 3, rate / 3, rate / 3) for _ in range(copies)]
            row = cs.call_groups(*as_groups(reads), qual_table=table)[0]
            assert row["status"] == cs.CALLED
            q = np.frombuffer(row["quality"], dtype=np.uint8)
            wrong, omitted = judge(orig.encode(), row["sequence"])
            expected += cs.expected_errors(row["quality"])[0]
            n_wrong += int(wrong.sum())
            n_omitted += omitted
            n_bases += q.size
            q_wrong += q[wrong].tolist()
            q_right += q[~wrong].tolist()
            for value in np.unique(q):
                cell = by_q.setdefault(int(value), [0, 0])
                cell[0] += int((q == value).sum())
                cell[1] += int(wrong[q == value].sum())
        say("   %4.0f %%  %6d  %6d  %10.2f  %12d  %14d  %13s  %13.1f" % (
            rate * 100, copies, n_bases, expected, n_wrong, n_omitted, "%.1f" % np.mean(q_wrong) if q_wrong else "-", np.mean(q_right)))
        tot_expected += expected
        tot_wrong += n_wrong
        tot_omitted += n_omitted
        tot_bases += n_bases
say("   all cells      %6d  %10.2f  %12d  %14d" % (tot_bases, tot_expected, tot_wrong, tot_omitted))
say("")
say("2. per quality value, all cells together")
say("   q    bases    wrong   counted error rate   claimed 10^(-q/10)   counted as Phred")
for value in sorted(by_q):
    n, w = by_q[value]
    say("   %2d  %7d  %7d   %18.5f   %18.6f   %s" % (value, n, w, w / n, 10 ** (-value / 10), "%.1f" % (-10 * np.log10(w / n)) if w else "no wrong base"))
say("   (%.0f s)" % (time.time() - t0))
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
