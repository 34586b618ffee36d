"""Seeded UMI adapters and end windows for the UMI tests (TEST INFRASTRUCTURE; no GPU): adapters with their degenerate rows at
row 0, at the last row, in a single row or over the whole adapter, and windows that carry an instance of the adapter whole,
edited, clipped by either window edge or not at all.  Returns strings and numpy arrays only."""
import random

import numpy as np

from tests import wild_ref

SCHEMES = {"default": (3, -6, -5, -2), "linear": (3, -6, -5, -5), "refused": (300, -600, -500, -200)}
PLACEMENTS = ("row0", "last", "single", "whole")
UMI28 = "TTTVVVVTTVVVVTTVVVVTTVVVVTTT"
UMI67 = "CAAGCAGAAGACGGCATACGAGAT" + UMI28 + "GTGACTGGAGTTCAG"
DEGENERATE = "RYSWKMBDHVN"
END_SIZE = 150


def adapter(rng, m, placement):
    """m rows, fixed letters A/C/G/T but for the degenerate rows of the placement."""
    rows = [rng.choice("ACGT") for _ in range(m)]
    k = max(1, m // 3)
    where = {"row0": range(0, k), "last": range(m - k, m), "single": [m // 2], "whole": range(m)}[placement]
    for r in where:
        rows[r] = rng.choice(DEGENERATE)
    return "".join(rows)


def instance(rng, ad):
    """One sequence the adapter matches: per row a member of its letter set."""
    out = []
    for ch in ad:
        s = wild_ref.letter_set(ord(ch), True)
        out.append(rng.choice([b for k, b in enumerate("ACGT") if s >> k & 1]))
    return "".join(out)


def edited(rng, seq, edits):
    seq = list(seq)
    for _ in range(edits):
        if not seq:
            break
        at = rng.randrange(len(seq))
        kind = rng.choice("SID")
        if kind == "S":
            seq[at] = rng.choice([b for b in "ACGT" if b != seq[at]])
        elif kind == "I":
            seq.insert(at, rng.choice("ACGT"))
        else:
            del seq[at]
    return "".join(seq)


def noise(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def window(rng, ad, length, how):
    """A window of `length` bases.  how: 'whole' (an instance with noise around it, cut to length wherever it falls),
    'edited', 'head' (the window starts inside the instance), 'tail' (it ends inside it), 'flush_end' (the instance ends at the
    window's last base), 'flush_start', 'absent'."""
    if length == 0:
        return ""
    inst = instance(rng, ad)
    if how == "edited":
        inst = edited(rng, inst, rng.randint(1, 3))
    if how == "absent":
        s = noise(rng, length, "ACGTACGTN")
    elif how == "head":
        s = inst[rng.randrange(len(inst)):] + noise(rng, length)
    elif how == "tail":
        s = noise(rng, length) + inst[:rng.randint(1, len(inst))]
        s = s[-length:]
    elif how == "flush_end":
        s = (noise(rng, length) + inst)[-length:]
    elif how == "flush_start":
        s = inst + noise(rng, length)
    else:
        lead = rng.randint(0, max(0, length - len(inst)))
        s = noise(rng, lead) + inst + noise(rng, length)
    return s[:length]


HOWS = ("whole", "edited", "head", "tail", "flush_end", "flush_start", "absent")


def lay_out(windows, alignments=None):
    """Windows laid into one arena, window k starting at a byte with offset % 4 == alignments[k] (random bytes between them;
    the arena ends with the last window's last byte).  -> (arena bytes, off int64, len int32)"""
    rng = random.Random(len(windows))
    parts, off, pos = [], [], 0
    for k, w in enumerate(windows):
        want = (k if alignments is None else alignments[k]) % 4
        pad = (want - pos) % 4
        parts.append(noise(rng, pad))
        pos += pad
        off.append(pos)
        parts.append(w)
        pos += len(w)
    if windows and not windows[-1]:
        parts.append("A")
    return "".join(parts).encode(), np.array(off, dtype=np.int64), np.array([len(w) for w in windows], dtype=np.int32)


def many_windows(seed, ad, count):
    """count windows of 0..150 bases for one adapter, every way of planting in turn; some are built to fail exactly one
    condition of phase B's rule (tests/test_gpu_umi.py counts them)."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        how = HOWS[k % len(HOWS)]
        length = END_SIZE if k % 3 == 0 else rng.randint(0, END_SIZE)
        if k % 50 == 7:
            out.append(instance(rng, ad)[:3])                  # a perfect alignment of three columns: below min_trim_size
        elif k % 97 == 5:
            out.append("")                                     # an empty window: no alignment
        else:
            out.append(window(rng, ad, length, how))
    return out
