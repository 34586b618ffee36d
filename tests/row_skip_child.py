"""The scan-level checks of tests/test_gpu_row_skip.py, run as a child process (TEST INFRASTRUCTURE):
    python -m tests.row_skip_child
started with PC_JIT_MIN_CELLS=1 so that the specialised packed-fp16 score kernels -- and, for a floored call, their
row-skipping variants (csrc/pc_bounds.h, row_skip_plan) -- run from the first launch.  Floored two-pass calls with the
skip against the same call under PC_NO_ROW_SKIP=1 (read per call), against the unfloored call and against the oracle:
pairs at or above their floor F have all eight record ints equal, pairs below have the "no alignment" record on both
sides, pc_floor_skipped is equal.  The batches plant what can go wrong: scores of exactly F and F - 1, copies starting at
each residue mod 4 of the column block, in column 1 and cut by the read's start, ending in the last column and hanging over
the read's end, two copies closer than W_low and just farther, one straddling the shortest read's end in a ragged tile, one
at each chunk boundary under PC_FORCE_CHUNKS=4, the widest one-gap copies, a tile with no copy at all and a tile of copies
only."""
import ctypes
import os
import random
import sys

import numpy as np
import torch

import porechop_amd
from oracle.oracle import Oracle
from porechop_amd.batch import MODE_TWO_PASS
from tests import floorgen, stretchgen

SENTINEL = np.array([-1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)
SCORES = floorgen.SCORES
THRESHOLD = 85.0                                            # (lower than the 90 % the rule for r0 is tuned to: more triggers)
R0 = 20                                                     # both headline pairs (tests/test_row_skip_host.py pins it)


def w_low(R, ms, floors):
    g = min(-SCORES[2], -SCORES[3])
    return (R - R0) + max((SCORES[0] * m - f) // g for m, f in zip(ms, floors))


def jit_stats(al):
    c, d = ctypes.c_int64(0), ctypes.c_int64(0)
    al.lib.pc_jit_stats(ctypes.byref(c), ctypes.byref(d))
    return c.value, d.value


class Batch:
    """n reads against the four middle adapters (33 | 30, 28 | 22): the oracle's scores and strings, once."""

    def __init__(self, oracle, reads):
        self.ads = [a[1] for a in floorgen.middle_adapters()]
        self.floors = [floorgen.score_bound(len(s), THRESHOLD) for s in self.ads]
        self.reads = reads
        self.n = len(reads)
        self.lens = np.array([len(r) for r in reads], dtype=np.int32)
        self.offs = np.concatenate([[0], np.cumsum(self.lens[:-1].astype(np.int64))]).astype(np.int64)
        self.arena = np.frombuffer(("".join(reads)).encode() + b"N" * 64, dtype=np.uint8).copy()
        ad_arena = np.frombuffer("".join(self.ads).encode(), dtype=np.uint8)
        ad_len = np.array([len(s) for s in self.ads], dtype=np.int32)
        ad_off = np.concatenate([[0], np.cumsum(ad_len[:-1].astype(np.int64))]).astype(np.int64)
        A = len(self.ads)
        o = oracle.align_many(self.arena, np.tile(self.offs, A), np.tile(self.lens, A), ad_arena, np.repeat(ad_off, self.n),
                              np.repeat(ad_len, self.n), SCORES).reshape(A, self.n, 9)
        self.score = o[:, :, 4].astype(np.int64)
        self.below = self.score < np.array(self.floors, dtype=np.int64)[:, None]
        self.max_len = int(self.lens.max())
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = (torch.from_numpy(self.arena).cuda(), torch.from_numpy(self.offs).cuda(), torch.from_numpy(self.lens).cuda())
        return self._dev


def planted(rng, ads, ln, which, edits):
    """ln random bases with one copy of each adapter in `which`, `edits` random edits each, well apart."""
    body = list(floorgen.random_bases(rng, ln))
    slots = list(range(len(which)))
    rng.shuffle(slots)
    for a, k in zip(which, slots):
        copy = floorgen.edit(rng, ads[a], rng.randint(0, edits))
        pos = 20 + k * ((ln - 80) // max(1, len(which))) + rng.randint(0, 15)
        body[pos:pos + len(copy)] = copy
    return "".join(body)[:ln]


def mixed_batch(oracle, seed, ragged):
    rng = random.Random(seed)
    ads = [a[1] for a in floorgen.middle_adapters()]
    floors = [floorgen.score_bound(len(s), THRESHOLD) for s in ads]
    n = 193                                                  # three 64-window tiles and one lane
    lens = [rng.randint(300, 1900) if ragged else 1000 for _ in range(n)]
    if ragged:
        lens[7] = 300                                        # the shortest read of tile 0: its end is nmin
    reads = [planted(rng, ads, lens[i], [0, 1, 2, 3], 2) if i % 2 == 0 else floorgen.random_bases(rng, lens[i]) for i in range(n)]

    def put(i, pos, piece):
        r = reads[i]
        reads[i] = (r[:pos] + piece + r[pos + len(piece):])[:len(r)] if pos >= 0 else (piece[-pos:] + r[len(piece) + pos:])
        assert len(reads[i]) == len(r)

    # scores of exactly F and F - 1 (the two sides of the comparison)
    exact = []
    for k, a in enumerate((0, 2, 3)):
        for d in (0, 1):
            slot = 3 + 31 * (2 * k + d)
            reads[slot] = floorgen.read_with_score(oracle, rng, ads[a], floors[a] - d, len(reads[slot]))
            exact.append((a, slot, floors[a] - d))
    # a copy starting at each residue mod 4 of the block, of each adapter
    for k in range(4):
        reads[67 + 2 * k] = floorgen.random_bases(rng, lens[67 + 2 * k])
        for a in range(4):
            put(67 + 2 * k, 40 + 60 * a + k, ads[a])
    # in column 1; cut by the read's start; ending in the last column; hanging over the read's end
    put(75, 0, ads[2]); put(77, -13, ads[0]); put(79, lens[79] - len(ads[1]), ads[1]); put(81, lens[81] - 22, ads[0])
    # two copies closer than W_low and just farther (28 | 22: W_low from the floors)
    w = w_low(28, (28, 22), floors[2:])
    put(83, 100, ads[2]); put(83, 100 + 28 + w - 6, ads[2]); put(83, 100 + 2 * 28 + 2 * w + 2, ads[3])
    # the widest one-gap copies: a run of filler bases in the middle, as long as the floor allows
    for i, a in ((85, 0), (87, 1), (89, 2), (91, 3)):
        m = len(ads[a])
        L = (SCORES[0] * m - floors[a] + SCORES[2]) // -SCORES[3] + 1
        put(i, 150, stretchgen.stretched(ads[a], [m // 2], L))
    if ragged:
        put(9, 300 - 12, ads[2])                             # straddles the end of the shortest read of its tile
    else:
        for c in (250, 500, 750):                            # each chunk boundary under PC_FORCE_CHUNKS=4
            put(93, c - 14, ads[2]); put(95, c - 3, ads[1])
    b = Batch(oracle, reads)
    for a, slot, want in exact:
        assert b.score[a, slot] == want
    return b


def scan(al, b, floors=None):
    arena, off, ln = b.dev
    n = b.n
    out = torch.full((4 * n, 8), 77, dtype=torch.int32, device="cuda")
    kw = {} if floors is None else dict(floors=[floors[0], floors[2]], floors_b=[floors[1], floors[3]])
    al.set_length_hint(int(b.lens.mean()) if b.lens.min() != b.lens.max() else 0)
    al.scan_device(arena, torch.cat([off, off]), torch.cat([ln, ln]), np.array([0, 2], dtype=np.int32), np.array([0, n, 2 * n], dtype=np.int64),
                   b.max_len, out, MODE_TWO_PASS, job_adapter_b=np.array([1, 3], dtype=np.int32), **kw)
    al.sync()
    return out.cpu().numpy().reshape(4, n, 8)


def both_ways(al, b, floors, what):
    """the floored call with the skip and without -> (records, on-fraction counters)"""
    os.environ["PC_NO_ROW_SKIP"] = "1"
    try:
        plain = scan(al, b, floors)
        skipped_plain = al.floor_skipped()[0]
        assert al.row_skip_blocks() == (0, 0), (what, "PC_NO_ROW_SKIP=1 ran a row-skipping launch")
    finally:
        del os.environ["PC_NO_ROW_SKIP"]
    got = scan(al, b, floors)
    blocks = al.row_skip_blocks()
    assert al.floor_skipped()[0] == skipped_plain, (what, al.floor_skipped(), skipped_plain)
    bad = np.nonzero((got != plain).any(axis=2))
    assert bad[0].size == 0, (what, "%d records differ" % bad[0].size, [(int(a), int(i), got[a, i].tolist(), plain[a, i].tolist())
                                                                      for a, i in list(zip(*bad))[:3]])
    return got, blocks


def run_mixed(al, oracle, b, what):
    base = scan(al, b)
    assert (base[:, :, 0] != -1).all() and (base[:, :, 4] == b.score).all(), (what, "the unfloored call against the oracle's scores")
    # by the oracle alone: a quarter of the pairs at or above F, a quarter below
    assert (~b.below).sum() * 4 >= b.below.size and b.below.sum() * 4 >= b.below.size, (what, int(b.below.sum()), b.below.size)
    got, (blocks, on) = both_ways(al, b, b.floors, what)
    assert (got[b.below] == SENTINEL).all() and (got[~b.below] == base[~b.below]).all(), what
    assert al.floor_skipped()[0] == int(b.below.sum()), what
    assert 0 < on < blocks, (what, on, blocks)               # the lower rows neither always on nor never
    # the records of the planted reads as the oracle's strings
    for i in list(range(67, 97, 2)) + [3, 34]:
        for a in range(4):
            if not b.below[a, i]:
                assert porechop_amd.format_result(got[a, i]) == oracle.adapter_alignment(b.reads[i], b.ads[a], SCORES), (what, a, i)
    return blocks, on


def main():
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1" and "PC_DISABLE_JIT" not in os.environ and "PC_NO_ROW_SKIP" not in os.environ
    o = Oracle()
    ads = [a[1] for a in floorgen.middle_adapters()]
    al = porechop_amd.Aligner(ads + ["GGTTGTTTCTGTTGGTGCTGATAT"], SCORES)
    al.set_row_skip_debug(True)
    before = jit_stats(al)
    uniform, ragged = mixed_batch(o, 21, False), mixed_batch(o, 22, True)
    print("ROW_SKIP uniform blocks=%d on=%d" % run_mixed(al, o, uniform, "uniform"))
    print("ROW_SKIP ragged blocks=%d on=%d" % run_mixed(al, o, ragged, "ragged"))
    st = jit_stats(al)
    # two pairs, each kernel and its row-skipping variant; that the variant -- packed fp16, there is no other -- is what ran is
    # pinned by the counters above: only its launches count blocks
    assert st[0] + st[1] - before[0] - before[1] >= 4, (before, st)
    os.environ["PC_FORCE_CHUNKS"] = "4"
    try:
        _, (blocks, on) = both_ways(al, uniform, uniform.floors, "four chunks")
        assert 0 < on < blocks, ("four chunks", on, blocks)     # the chunks' launches were row-skipping ones
    finally:
        del os.environ["PC_FORCE_CHUNKS"]
    # a pair for which the host refuses: floors that leave theta <= 0 (the column-0 condition) -- the plain launches, same records
    low = [20, 20, 12, 12]
    got, (blocks, on) = both_ways(al, uniform, low, "refused")
    assert (blocks, on) == (0, 0), ("refused floors ran a row-skipping launch", blocks, on)
    # a tile with no copy at all: the lower rows never switch on (the counters leave out the untriggered first window of a
    # stretch of blocks, which computes them whatever the reads hold)
    # (reads of N, which match nothing: among random bases a gapped prefix alignment reaches theta of the shorter half in about
    # one column of two thousand, so that a tile of random reads does switch them on now and then)
    rng = random.Random(5)
    empty = Batch(o, ["N" * 1000 for _ in range(64)])
    assert empty.below.all()
    got, (blocks, on) = both_ways(al, empty, empty.floors, "empty tile")
    assert (got == SENTINEL).all()
    assert blocks > 0 and on == 0, ("empty tile", blocks, on)
    # a tile of random reads at the floors of the default 90 %, which the rule for r0 is made for: the lower part of a block
    # costs 365 instructions (28 | 22) and 502 (33 | 30) where skipping saves 207 and 311 (profiles/score_row_skip_audit.txt),
    # so past an on-fraction of 207 / 365 = 0.57 the skip would lose; random reads must stay under half of that
    noise = Batch(o, [floorgen.random_bases(rng, 1000) for _ in range(64)])
    floors90 = [floorgen.score_bound(len(s), 90.0) for s in noise.ads]
    got, (blocks, on) = both_ways(al, noise, floors90, "random reads")
    print("ROW_SKIP random reads at 90 %%: blocks=%d on=%d" % (blocks, on))
    assert blocks > 0 and on < 0.28 * blocks, ("random reads", blocks, on)
    # a tile of copies only, one every 20 columns: the lower rows on in every block
    body = "".join((ads[k % 4] + floorgen.random_bases(rng, 3))[:20 + (k % 3)] for k in range(60))[:1000]
    full = Batch(o, [(ads[i % 4] + body)[:1000] for i in range(64)])
    got, (blocks, on) = both_ways(al, full, full.floors, "copies only")
    assert blocks > 0 and on == blocks, ("copies only", blocks, on)
    # one single 24-mer: a job of its own (two read streams per lane)
    arena, off, ln = uniform.dev
    n = uniform.n
    reads24 = list(uniform.reads)
    f24 = floorgen.score_bound(24, THRESHOLD)
    outs = []
    for env in ("1", None):
        if env:
            os.environ["PC_NO_ROW_SKIP"] = env
        else:
            os.environ.pop("PC_NO_ROW_SKIP", None)
        out = torch.full((n, 8), 77, dtype=torch.int32, device="cuda")
        al.scan_device(arena, off, ln, np.array([4], dtype=np.int32), np.array([0, n], dtype=np.int64), uniform.max_len, out, MODE_TWO_PASS,
                       floors=[f24])
        al.sync()
        outs.append((out.cpu().numpy(), al.floor_skipped()[0], al.row_skip_blocks()))
    os.environ.pop("PC_NO_ROW_SKIP", None)
    assert (outs[0][0] == outs[1][0]).all() and outs[0][1] == outs[1][1] and outs[0][2] == (0, 0) and outs[1][2][0] > 0, [x[1:] for x in outs]
    assert len(reads24) == n
    al.close()
    print("ROW_SKIP_CHILD_OK")


if __name__ == "__main__":
    sys.exit(main())
