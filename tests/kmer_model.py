"""The k-mer census in plain numpy: the model of pc_kmer_count (include/porechop_amd.h) for the discovery tests.

A k-mer's code holds 2 bits per base, the first base in the highest bits: A 0, C 1, G 2, T 3, U as T, either case (SeqAn's
Dna order, porechop/include/seqan/basic/alphabet_residue_tabs.h:113-140).  A k-mer that covers any other byte is not counted.
Counting only adds."""
import random

import numpy as np

CODE = np.full(256, 4, dtype=np.int64)
for _i, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _ch in _letters:
        CODE[ord(_ch)] = _i


def kmer_codes(windows, k):
    """Every countable k-mer of every window (bytes / str) -> int64 codes, with repeats."""
    parts = []
    for w in windows:
        b = w.encode() if isinstance(w, str) else bytes(w)
        parts.append(np.frombuffer(b, dtype=np.uint8))
        parts.append(np.zeros(1, dtype=np.uint8))             # a non-base between windows: no k-mer spans two of them
    if not parts:
        return np.zeros(0, dtype=np.int64)
    c = CODE[np.concatenate(parts)]
    m = c.size - k + 1
    if m <= 0:
        return np.zeros(0, dtype=np.int64)
    code = np.zeros(m, dtype=np.int64)
    bad = np.zeros(m, dtype=bool)
    for i in range(k):
        code = (code << 2) | (c[i:i + m] & 3)
        bad |= c[i:i + m] == 4
    return code[~bad]


def count_sparse(windows, k):
    """-> (codes ascending, counts), the nonzero entries of the table"""
    return np.unique(kmer_codes(windows, k), return_counts=True)


def count_dense(windows, k, counts=None):
    """-> the dense int64[4^k] table; counts given: added to (and returned)"""
    if counts is None:
        counts = np.zeros(1 << (2 * k), dtype=np.int64)
    counts += np.bincount(kmer_codes(windows, k), minlength=counts.size)
    return counts


def encode(kmer):
    v = 0
    for ch in kmer:
        v = (v << 2) | int(CODE[ord(ch)])
    return v


# ---- the planted-adapter reads of the recovery tests -------------------------------------------------------------------
Y_TOP, Y_BOTTOM = "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"


def mutate(rng, seq, e):
    """Each base with probability e: a third each a random substitution, a deletion, an insertion after it."""
    out = []
    for ch in seq:
        if rng.random() < e:
            kind = rng.randrange(3)
            if kind == 0:
                out.append(rng.choice([b for b in "ACGT" if b != ch]))
            elif kind == 2:
                out.append(ch)
                out.append(rng.choice("ACGT"))
        else:
            out.append(ch)
    return "".join(out)


def planted_reads(n, f, e, seed, start=Y_TOP, end=Y_BOTTOM):
    """n reads: a body of 200-599 uniform random bases; with probability f each, the start adapter behind 0-11 random bases
    and the end adapter before 0-11 random bases, every adapter base mutated with probability e."""
    rng = random.Random(seed)

    def rand(m):
        return "".join(rng.choice("ACGT") for _ in range(m))
    reads = []
    for _ in range(n):
        r = rand(rng.randrange(200, 600))
        if rng.random() < f:
            r = rand(rng.randrange(12)) + mutate(rng, start, e) + r
        if rng.random() < f:
            r = r + mutate(rng, end, e) + rand(rng.randrange(12))
        reads.append(r)
    return reads


def end_windows(reads, end_size=150):
    """-> (start windows, end windows) as phase B cuts them"""
    return [r[:end_size] for r in reads], [r[-end_size:] for r in reads]
