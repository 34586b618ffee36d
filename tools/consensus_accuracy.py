#!/usr/bin/env python3
"""Accuracy record of the UMI consensus rule on the HOST MODEL (porechop_amd.consensus: numpy, no GPU):
  1. identity of the consensus to the original, by group size {3, 5, 10, 20} and error rate {5, 10 %} (a third each of
     substitutions, insertions and deletions) on originals of 1 kb, defaults otherwise (band 64, two rounds, 30 %): the mean and
     the worst of `trials` seeded groups, beside the identity of the groups' best member;
  2. the check on the band default: pairs of two independent copies of one 8 kb original, at three error rates; per band 32, 64
     and 128 the share of pairs whose path leaves the band (the banded distance exceeds that at band 1024) and the share the
     rule rejects (distance * 100 > 30 * length).
Seeded: the same numbers every time.  A record, not a gate.
   python tools/consensus_accuracy.py [trials] [pairs] [out.txt]      (default 5, 32, profiles/consensus_accuracy.txt)"""
import random
import sys
import time
sys.path.insert(0, ".")
import numpy as np
from porechop_amd import consensus as cs

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 5
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 32
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/consensus_accuracy.txt"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def original(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def copy_of(rng, seq, sub, ins, dele):
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


def distance(a, b, band=200):
    d, _ = cs.align(cs.codes(a), cs.codes(b), band)
    return d


def as_groups(reads):
    off = np.concatenate([[0], np.cumsum([len(s) + 1 for s in reads])])[:-1].astype(np.int64)
    arena = np.frombuffer(b"".join(s + b"-" for s in reads), dtype=np.uint8)
    return [(1, "K", list(range(len(reads))))], arena, off, np.array([len(s) for s in reads], dtype=np.int64)


t0 = time.time()
say("UMI consensus, host model (porechop_amd.consensus), defaults: band %(band)d, rounds %(rounds)d, max_err_pct %(max_err_pct)d, min_reads %(min_reads)d" % cs.DEFAULTS)
say("")
say("1. identity to the original (1 - edit distance / 1000), originals of 1 kb, %d seeded groups per cell" % trials)
say("   errors  copies   consensus mean   consensus worst   best member mean   called")
for rate in (0.05, 0.10):
    for copies in (3, 5, 10, 20):
        got, best, called = [], [], 0
        for trial in range(trials):
            rng = random.Random(1000 * copies + int(rate * 100) * 10 + trial)
            orig = original(rng, 1000)
            reads = [copy_of(rng, orig, rate / 3, rate / 3, rate / 3) for _ in range(copies)]
            out = cs.call_groups(*as_groups(reads))[0]
            best.append(1 - min(distance(orig.encode(), r) for r in reads) / 1000)
            if out["status"] == cs.CALLED:
                called += 1
                got.append(1 - distance(orig.encode(), out["sequence"]) / 1000)
        say("   %4.0f %%  %6d   %14.4f   %15.4f   %16.4f   %d/%d" % (rate * 100, copies, np.mean(got) if got else float("nan"),
                                                                       min(got) if got else float("nan"), np.mean(best), called, trials))
say("   (%.0f s)" % (time.time() - t0))
say("")
t0 = time.time()
say("2. the band: %d pairs of two independent copies of one 8 192-base original per error rate" % pairs)
say("   errors per copy (sub / ins / del)   band   path leaves the band   rejected at 30 %   mean distance / length")
for sub, ins, dele in ((0.02, 0.02, 0.02), (0.025, 0.025, 0.025), (0.05, 0.05, 0.05)):
    rng = random.Random(int(sub * 1000) + 8192)
    made = []
    for _ in range(pairs):
        orig = original(rng, 8192)
        made.append((copy_of(rng, orig, sub, ins, dele), copy_of(rng, orig, sub, ins, dele)))
    wide = [distance(a, b, 1024) for a, b in made]
    for band in (32, 64, 128):
        d = [distance(a, b, band) for a, b in made]
        left = sum(1 for x, w in zip(d, wide) if x > w)
        rej = sum(1 for x, (a, b) in zip(d, made) if cs.rejected(x, len(a), len(b), 30))
        say("   %4.1f / %4.1f / %4.1f %%                  %4d   %9d / %-8d   %8d / %-6d   %.4f" % (
            sub * 100, ins * 100, dele * 100, band, left, pairs, rej, pairs, float(np.mean([x / max(len(a), len(b)) for x, (a, b) in zip(d, made)]))))
say("   (%.0f s)" % (time.time() - t0))
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
