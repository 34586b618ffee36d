"""Barcode discovery in plain numpy: the model of pc_anchor_inserts (include/porechop_amd.h) from scan records, and the
barcoded reads of the recovery tests.

A window is anchored iff rec[0] >= 0, rec[7] > 0, 100 * rec[5] >= min_identity * rec[7] and the alignment reaches the anchor's
inner edge (side 0: rec[3] == anchor_len - 1; side 1: rec[2] == 0).  The insert begins at col = rec[1] + 1 (side 0) or
rec[0] - L (side 1); its code holds 2 bits per base, the first base in the highest bits (tests/kmer_model.py's CODE), and is
-1 where the window is not anchored, the insert does not lie inside the window or holds a byte that is not a base."""
import random

import numpy as np

from tests import kmer_model as km

# the two fixed strings of tests/test_gpu_discover.py
A_S, A_E = "GTCACGGAGATCCCCGTACGGGGTAGACCA", "AAAGGCATTTCCCTCCCATATAAG"


def anchor_inserts(arena, win_off, win_len, records, anchor_len, side, min_identity=75, insert_len=24):
    """arena uint8[*], win_off int64[n], win_len int32[n], records int32[n, 8] -> int64[n] (Python integers wrapped to 64
    bits, as the library's uint64 -> int64 does at insert_len = 32)"""
    arena = np.asarray(arena, dtype=np.uint8)
    records = np.asarray(records).reshape(-1, 8)
    L = int(insert_len)
    out = np.full(records.shape[0], -1, dtype=np.int64)
    for w, (off, n, rec) in enumerate(zip(np.asarray(win_off).tolist(), np.asarray(win_len).tolist(), records.tolist())):
        if rec[0] < 0 or rec[7] <= 0 or 100 * rec[5] < int(min_identity) * rec[7]:
            continue
        if (rec[3] != int(anchor_len) - 1) if side == 0 else (rec[2] != 0):
            continue
        col = rec[1] + 1 if side == 0 else rec[0] - L
        if col < 0 or col + L > n:
            continue
        codes = km.CODE[arena[off + col:off + col + L]].tolist()
        if 4 in codes:
            continue
        v = 0
        for c in codes:
            v = (v << 2) | c
        out[w] = v - (1 << 64) if v >= 1 << 63 else v
    return out


def rc(seq):
    return seq[::-1].translate(str.maketrans("ACGT", "TGCA"))


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def make_barcodes(nb, L, seed):
    """nb random L-mers, each accepted only with edit distance >= 8 to every earlier one and to its reverse complement"""
    rng = random.Random(seed)
    out = []
    while len(out) < nb:
        c = "".join(rng.choice("ACGT") for _ in range(L))
        if all(edit_distance(c, x) >= 8 and edit_distance(c, rc(x)) >= 8 for x in out):
            out.append(c)
    return out


def barcoded_reads(n, barcodes, e, seed, f=0.8, flank="CAGCACCT"):
    """n reads: a body of 200-599 random bases; one barcode per read, drawn uniformly; with probability f each, the start
    rand(0..11) + mutate(A_S + bc + flank, e) and the end mutate(rc(flank) + rc(bc) + A_E, e) + rand(0..11)
    -> (reads, index of each read's barcode)"""
    rng = random.Random(seed)

    def rand(m):
        return "".join(rng.choice("ACGT") for _ in range(m))
    reads, which = [], []
    for _ in range(n):
        b = rng.randrange(len(barcodes))
        r = rand(rng.randrange(200, 600))
        if rng.random() < f:
            r = rand(rng.randrange(12)) + km.mutate(rng, A_S + barcodes[b] + flank, e) + r
        if rng.random() < f:
            r = r + km.mutate(rng, rc(flank) + rc(barcodes[b]) + A_E, e) + rand(rng.randrange(12))
        reads.append(r)
        which.append(b)
    return reads, which
