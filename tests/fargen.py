"""Seeded placements of one small block of read windows at far offsets of a 4.3 GB arena (TEST INFRASTRUCTURE; no GPU).

Every kernel of the library takes int64 offsets and must carry them in 64 bits to the load or store.  To check that
without filling gigabytes, ONE block of 131 windows laid back to back, plus 2 sub-windows (133 listed, under 64 KB), is
placed four times in an arena that is otherwise never written:

    near      at byte 0
    cross31   byte 2^31 falls inside the planted adapter copy of the designated window
    cross32   byte 2^32 falls inside that copy
    beyond32  the block starts at 2^32 + 2^20 + 1 (odd): window starts take every residue mod 64

Besides the back-to-back windows the block lists two SUB-WINDOWS of the designated window D, cut inside its planted copy:
D[:split] and D[split:].  They overlap D (the scans and the prefilter only read), and at the crossing placements the first
ends in the byte before the boundary and the second starts on it: a window-to-window boundary and a boundary inside a
window, in one placement.  `Block.disjoint` lists the windows without D: ascending and not overlapping, what
pc_unpack_windows asks for.

Before each placed block lie at least 4 KB of random bytes and behind it 128 (the kernels legitimately read there: a
lead-in before a window, 16-byte fetches past its end, the 512-base line below a packed window); they differ per placement.
The lead is as long as it takes for the placement's image (lead + block + tail) to start on a multiple of 64 bases, so the
image can be packed on its own (pack_reads) and copied into a 2-bit plane at image_start // 4.

This module returns byte strings and offsets only."""
import random

import numpy as np

from tests.pairgen import mutate

B31, B32 = 1 << 31, 1 << 32
ARENA_BYTES = B32 + (1 << 21)
PLANE_BYTES = ARENA_BYTES // 4 + 64
LEAD, TAIL = 4096, 128
PLACEMENTS = ("near", "cross31", "cross32", "beyond32")
BEYOND32_START = B32 + (1 << 20) + 1
# 131 back-to-back windows (the block lists 133: two sub-windows of the designated one are added): one dual tile of 64,
# one single-adapter tile of 128 and a ragged rest
LENGTHS = [2500] * 2 + [700] * 5 + [1, 1, 3, 3, 16, 16, 17, 17] + [149] * 6 + [151] * 6 + [150] * 104
ALPHABETS = ["ACGT", "ACGT", "ACGT", "ACGTN-", "acgtACGTUu"]
RATES = [0.0, 0.05, 0.15]


SEED = 2032
SCORES = (3, -6, -5, -2)
THRESHOLDS = (90.0, 85.0, 70.0)
Y_TOP, Y_BOTTOM = "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"


def far_adapters():
    """-> (dp, nine, long200, every sequence once): the DP scans' adapters from the committed panel -- a 33-, 30-, 28-, 22- and
    24-mer, so that their specialised kernels are in the built cache --, the nine adapters of tests/test_gpu_packed_total.py
    for the prefilter, and a 200-base adapter for the plain-int32 kernel's HBM state."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panel.json")) as f:
        panel = json.load(f)
    seqs = []
    for s in panel:
        for x in (s["start"], s["end"]):
            if x is not None and x[1] not in seqs:
                seqs.append(x[1])
    dp = [next(q for q in seqs if len(q) == m) for m in (33, 30, 28, 22, 24)]
    assert dp[2] == Y_TOP and dp[3] == Y_BOTTOM
    rng = random.Random(5)
    nine = [Y_TOP, Y_BOTTOM] + ["".join(rng.choice("ACGT") for _ in range(m)) for m in (4, 10, 24, 30, 33, 38, 70)]
    rng = random.Random(200)
    long200 = "".join(rng.choice("ACGT") for _ in range(200))
    every = dp + [a for a in nine if a not in dp] + [long200]
    return dp, nine, long200, every


class Block:
    """data: the block's bytes; off / len: the windows (offsets from the block's first byte); reads: their strings;
    designated: index of D; copy: (first, last + 1) of D's planted copy inside D; split: where D is cut;
    sub: indices of D[:split] and D[split:]; disjoint: every window but D (ascending, not overlapping);
    planted: per window, the indices (into the adapter list) of the copies it carries."""

    def __init__(self, data, off, length, designated, copy, split, planted):
        self.data = data
        self.off = np.asarray(off, dtype=np.int64)
        self.len = np.asarray(length, dtype=np.int32)
        self.n = int(self.off.shape[0])
        self.designated, self.copy, self.split = designated, copy, split
        self.sub = (designated + 1, designated + 2)
        self.disjoint = [i for i in range(self.n) if i != designated]
        self.planted = planted
        text = data.decode("latin-1")
        self.reads = [text[o:o + l] for o, l in zip(self.off.tolist(), self.len.tolist())]
        self.max_len = int(self.len.max())


def _plant(rng, body, lo, hi, adapter, rate):
    """A mutated copy of `adapter` written over body[lo:hi], starting at a random column of it, cut at hi."""
    cp = mutate(rng, adapter, rate)[:hi - lo]
    if not cp:
        return None
    pos = lo + rng.randint(0, hi - lo - len(cp))
    body[pos:pos + len(cp)] = cp
    return pos, pos + len(cp)


def make_block(seed, adapters, acgt_only=False):
    """The block for `adapters` (every second window carries copies of up to eight of them, side by side, drawn as
    pairgen.mutate does at rates 0, 0.05 and 0.15).  acgt_only: the same windows with every letter that is not A/C/G/T replaced by one."""
    rng = random.Random(seed)
    lengths = list(LENGTHS)
    while True:                                   # an order in which the window starts take every residue mod 64
        rng.shuffle(lengths)
        if len(set((np.cumsum([0] + lengths[:-1]) % 64).tolist())) == 64:
            break
    designated = next(i for i, n in enumerate(lengths) if n == 700 and i > 20)
    windows, planted, copy, turn = [], [], None, 0
    for i, n in enumerate(lengths):
        alphabet = rng.choice(ALPHABETS)
        body = [rng.choice(alphabet) for _ in range(n)]
        mine = []
        if i == designated:
            while copy is None or copy[1] - copy[0] < 16:
                copy = _plant(rng, body, 300, 400, adapters[0], 0.05)
            mine.append(0)
        elif i % 2 == 0 and n >= 16:
            parts = min(n // 50, 8) if n >= 149 else 1             # copies side by side, ~50 columns each
            for lo, hi in [(n * q // parts, n * (q + 1) // parts) for q in range(parts)]:
                a = turn % len(adapters)
                turn += 1
                if _plant(rng, body, lo, hi, adapters[a], RATES[(turn // len(adapters) + a) % 3]) is not None:
                    mine.append(a)
        windows.append("".join(body))
        planted.append(mine)
    if acgt_only:
        fix = random.Random(seed + 1)
        windows = ["".join(c if c in "ACGT" else fix.choice("ACGT") for c in w.upper().replace("U", "T")) for w in windows]
    off, pos = [], 0
    for w in windows:
        off.append(pos)
        pos += len(w)
    split = (copy[0] + copy[1]) // 2
    length = [len(w) for w in windows]
    d = designated
    off[d + 1:d + 1] = [off[d], off[d] + split]
    length[d + 1:d + 1] = [split, length[d] - split]
    planted[d + 1:d + 1] = [[], []]
    return Block("".join(windows).encode("latin-1"), off, length, d, copy, split, planted)


class Layout:
    """start[name]: the byte the block's first byte sits at; lead[name] / tail[name]: the random bytes before and behind
    it; win_off / win_len: the windows of the four placements, placement by placement (4 * block.n of them)."""

    def __init__(self, block, seed):
        self.block = block
        at = int(block.off[block.designated]) + block.split
        self.start = {"near": 0, "cross31": B31 - at, "cross32": B32 - at, "beyond32": BEYOND32_START}
        rng = np.random.default_rng(seed)
        self.lead, self.tail = {}, {}
        for name in PLACEMENTS:
            s = self.start[name]
            self.lead[name] = rng.integers(0, 256, size=0 if s == 0 else LEAD + (s - LEAD) % 64, dtype=np.uint8).tobytes()
            self.tail[name] = rng.integers(0, 256, size=TAIL, dtype=np.uint8).tobytes()
        self.win_off = np.concatenate([block.off + self.start[name] for name in PLACEMENTS]).astype(np.int64)
        self.win_len = np.concatenate([block.len] * len(PLACEMENTS)).astype(np.int32)

    def image(self, name, block=None):
        """(first byte, bytes) of a placement: lead + block + tail.  `block`: a variant with the same windows."""
        block = self.block if block is None else block
        assert len(block.data) == len(self.block.data)
        return self.start[name] - len(self.lead[name]), self.lead[name] + block.data + self.tail[name]

    def rows(self, name):
        """The slice of win_off / win_len (and of every per-window result) that belongs to a placement."""
        k = PLACEMENTS.index(name)
        return slice(k * self.block.n, (k + 1) * self.block.n)

    def packed_images(self, block=None):
        """Per placement (first byte of the packed image in the plane, packed bytes, exception positions in bases of the
        whole arena), and all exception positions, ascending -- pack_reads over each image alone."""
        from porechop_amd.io import pack_reads
        out, exc_all = {}, []
        for name in PLACEMENTS:
            first, data = self.image(name, block)
            assert first % 64 == 0
            pk, exc = pack_reads(np.frombuffer(data, dtype=np.uint8))
            out[name] = (first // 4, pk, exc + first)
            exc_all.append(exc + first)
        exc_all = np.concatenate(exc_all).astype(np.int64)
        assert np.all(np.diff(exc_all) > 0)
        return out, exc_all


def make_layout(seed, adapters):
    """-> (layout of the block, the same block made of A/C/G/T only)"""
    block = make_block(seed, adapters)
    same = make_block(seed, adapters, acgt_only=True)
    assert np.array_equal(block.off, same.off) and np.array_equal(block.len, same.len)
    return Layout(block, seed), same
