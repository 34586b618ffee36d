"""The scan-level checks of tests/test_gpu_row_skip_top.py, run as a child process (TEST INFRASTRUCTURE):
    python -m tests.row_skip_top_child OUT.npz
started with PC_JIT_MIN_CELLS=1 and a kernel cache directory of its own, once with the default layout of the row-skipping score
kernels (the shorter adapter of a pair top-aligned: csrc/pc_bounds.h row_skip_plan_top) and once with PC_SKIP_LAYOUT=bottom.
Every case is a floored two-pass call with the skip, compared here with the same call under PC_NO_ROW_SKIP=1 (all records,
the floor counter) and with the oracle (pairs at or above their floor: the oracle's score, and its string for the first
forty of each adapter; pairs below: the "no alignment" record); the records go to OUT.npz, where the parent compares the
two layouts' runs with each other.  Built on tests/row_skip_child.py's batches and calls."""
import os
import random
import sys

import numpy as np
import torch

import porechop_amd
from oracle.oracle import Oracle
from porechop_amd.batch import MODE_TWO_PASS
from tests import floorgen
from tests.row_skip_child import SCORES, SENTINEL, THRESHOLD, Batch, both_ways, jit_stats, mixed_batch

EQUAL_A, EQUAL_B = "ACGGTCATTGCAGATCCGTTAGCAAT", "TTGCCAGTAGGCTAACGTCCATGAGA"      # 26 | 26: no kernel of the shipped panel


def check(al, oracle, b, floors, what, expect_on=None):
    """the floored call with the skip against the one without, and against the oracle -> its records"""
    below = b.score < np.array(floors, dtype=np.int64)[:, None]
    got, (blocks, on) = both_ways(al, b, floors, what)
    assert (got[below] == SENTINEL).all(), (what, "a pair below its floor has a record")
    assert (got[~below][:, 0] != -1).all() and (got[:, :, 4][~below] == b.score[~below]).all(), (what, "scores at or above the floor")
    for a in range(4):
        for i in np.nonzero(~below[a])[0][:40]:
            assert porechop_amd.format_result(got[a, i]) == oracle.adapter_alignment(b.reads[i], b.ads[a], SCORES), (what, a, int(i))
    if expect_on == "some":
        assert 0 < on < blocks, (what, on, blocks)
    print("TOP_CASE %s: %d pairs at or above, %d below, blocks=%d on=%d" % (what, int((~below).sum()), int(below.sum()), blocks, on))
    return got


def put(read, pos, piece):
    return (read[:pos] + piece + read[pos + len(piece):])[:len(read)]


def equal_length_pair(oracle, out, cache_dir):
    """a 26 | 26 pair of two different adapters: both layouts are one -- the same kernels by name in the cache, the same records"""
    rng = random.Random(77)
    ads = [EQUAL_A, EQUAL_B]
    reads = [floorgen.random_bases(rng, 600) for _ in range(128)]
    for i in range(0, 128, 2):
        reads[i] = put(reads[i], 50 + i, floorgen.edit(rng, ads[(i // 2) % 2], rng.randint(0, 3)))
        if i % 8 == 0:
            reads[i] = put(reads[i], 300 + i, ads[1 - (i // 2) % 2])
    floors = [floorgen.score_bound(26, THRESHOLD)] * 2
    al = porechop_amd.Aligner(ads, SCORES)
    al.set_row_skip_debug(True)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    arena = torch.from_numpy(np.frombuffer("".join(reads).encode() + b"N" * 64, dtype=np.uint8).copy()).cuda()
    off, ln = torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()
    n = len(reads)
    recs = {}
    for env in ("1", None):
        if env:
            os.environ["PC_NO_ROW_SKIP"] = env
        else:
            os.environ.pop("PC_NO_ROW_SKIP", None)
        o = torch.full((2 * n, 8), 77, dtype=torch.int32, device="cuda")
        al.scan_device(arena, off, ln, np.array([0], dtype=np.int32), np.array([0, n], dtype=np.int64), 600, o, MODE_TWO_PASS,
                       job_adapter_b=np.array([1], dtype=np.int32), floors=[floors[0]], floors_b=[floors[1]])
        al.sync()
        recs[env] = (o.cpu().numpy().reshape(2, n, 8), al.row_skip_blocks())
    # (the row-skipping variant ran and switched its lower rows on; how often is the headline pairs' business below)
    assert recs["1"][1] == (0, 0) and 0 < recs[None][1][1] <= recs[None][1][0], (recs["1"][1], recs[None][1])
    got = recs[None][0]
    assert (got == recs["1"][0]).all()
    hits = 0
    for a in range(2):
        for i in range(n):
            want = oracle.adapter_alignment(reads[i], ads[a], SCORES)
            if got[a, i, 0] != -1:
                assert porechop_amd.format_result(got[a, i]) == want, (a, i)
                hits += 1
    assert hits >= 64
    al.close()
    out["equal"] = got
    # the kernels this pair compiled, by the names the cache gives them (a hash of the source and the options)
    print("EQUAL_KERNELS " + " ".join(sorted(f for f in os.listdir(cache_dir) if f.endswith(".pcjk"))))


def main():
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1" and "PC_DISABLE_JIT" not in os.environ and "PC_NO_ROW_SKIP" not in os.environ
    cache_dir = os.environ["PC_JIT_CACHE_DIR"]
    bottom = os.environ.get("PC_SKIP_LAYOUT") == "bottom"
    o = Oracle()
    out = {}
    equal_length_pair(o, out, cache_dir)
    ads = [a[1] for a in floorgen.middle_adapters()]
    assert [len(s) for s in ads] == [33, 30, 28, 22]
    al = porechop_amd.Aligner(ads, SCORES)
    al.set_row_skip_debug(True)
    before = jit_stats(al)
    # ---- a uniform and a ragged tile (parked last column) with everything tests/row_skip_child.py plants; on-fraction 0 < on < all
    uniform, ragged = mixed_batch(o, 31, False), mixed_batch(o, 32, True)
    out["uniform"] = check(al, o, uniform, uniform.floors, "uniform", "some")
    out["ragged"] = check(al, o, ragged, ragged.floors, "ragged", "some")
    st = jit_stats(al)
    # the headline pairs' default kernels ship with the library; the bottom-aligned variants are this process's own
    if bottom:
        assert st[0] - before[0] >= 2, ("PC_SKIP_LAYOUT=bottom compiled nothing", before, st)
    else:
        assert st[0] - before[0] == 0, ("the default row-skipping kernels are not the shipped ones", before, st)
    # ---- forced chunks: c0 > 0 in every chunk but the first
    os.environ["PC_FORCE_CHUNKS"] = "4"
    try:
        out["chunks"] = check(al, o, uniform, uniform.floors, "four chunks", "some")
    finally:
        del os.environ["PC_FORCE_CHUNKS"]
    rng = random.Random(9)
    # ---- a hit in the short half only, in the long half only, in both inside one window (33 | 30 and 28 | 22), exact and edited
    reads = [floorgen.random_bases(rng, 700) for _ in range(192)]
    for i in range(192):
        kind, pair = i % 4, (i // 4) % 2
        long_ad, short_ad = ads[2 * pair], ads[2 * pair + 1]
        e = lambda s: floorgen.edit(rng, s, rng.randint(0, 2))
        if kind == 0:
            reads[i] = put(reads[i], 100 + i, e(short_ad))
        elif kind == 1:
            reads[i] = put(reads[i], 100 + i, e(long_ad))
        elif kind == 2:                                      # the second copy starts inside the first one's window
            reads[i] = put(put(reads[i], 100 + i, e(long_ad)), 100 + i + len(long_ad) + i % 9, e(short_ad))
    halves = Batch(o, reads)
    out["halves"] = check(al, o, halves, halves.floors, "halves", "some")
    # ---- the last column.  Reads that end inside a copy of each adapter (the alignment ends in the last column at a row < m),
    # and reads whose last chunk under PC_FORCE_CHUNKS=4 starts right behind an exact copy of the SHORT adapter and is only
    # k <= R - m_short columns long: the padding rows below the short adapter carry the copy's score into the last column,
    # above anything the chunk's real candidates hold (the copy's own end cell belongs to the chunk before).
    reads = []
    for i in range(128):
        a = i % 4
        cut = len(ads[a]) - 1 - (i // 4) % 6                 # rows m - 1 .. m - 6 in the last column
        body = floorgen.random_bases(rng, 400 + (i % 3))
        reads.append(body[:len(body) - cut] + ads[a][:cut])
    lastcol = Batch(o, reads)
    out["lastcol"] = check(al, o, lastcol, lastcol.floors, "last column")
    reads = [floorgen.random_bases(rng, 1000) for _ in range(64)]
    for i in range(64):
        short_ad = ads[1] if i % 2 else ads[3]
        k = 1 + (i // 2) % (3 if i % 2 else 6)
        if i >= 4:                                           # (reads 0 .. 3 keep the full length: max_len 1000, chunks of 250)
            r = floorgen.random_bases(rng, 750 + k)
            reads[i] = put(r, 750 - len(short_ad), short_ad)
    os.environ["PC_FORCE_CHUNKS"] = "4"
    try:
        behind = Batch(o, reads)
        out["behind"] = check(al, o, behind, behind.floors, "padding rows behind a lead-in")
    finally:
        del os.environ["PC_FORCE_CHUNKS"]
    # ---- reads of 1, 5, m_short - 1, m_short and m_short + 1 columns (both pairs' short adapters), copies where they fit
    reads = []
    for i in range(120):
        ln = (1, 5, 21, 22, 23, 29, 30, 31)[i % 8]
        src = ads[3] if ln <= 23 else ads[1]
        reads.append(src[:ln] + floorgen.random_bases(rng, max(0, ln - len(src))) if i % 3 else floorgen.random_bases(rng, ln))
    tiny = Batch(o, reads)
    out["tiny"] = check(al, o, tiny, tiny.floors, "tiny reads")
    # ---- exact copies at a threshold of 100 %: F = match * m, theta is reached exactly and every column of W_low is needed
    reads = [floorgen.random_bases(rng, 500) for _ in range(128)]
    for i in range(128):
        if i % 2 == 0:
            reads[i] = put(reads[i], 60 + i, ads[i // 2 % 4])
        if i % 8 == 0:
            reads[i] = put(reads[i], 300 + i % 50, ads[(i // 2 + 1) % 4])
    exact = Batch(o, reads)
    f100 = [SCORES[0] * len(s) for s in ads]
    out["exact"] = check(al, o, exact, f100, "exact copies at 100 %", "some")
    # ---- one tile of 2100-column windows: the renormalisation (every 1928 / 1912 columns) falls inside an open window
    reads = [floorgen.random_bases(rng, 2100) for _ in range(64)]
    for i in range(64):
        a = i % 4
        reads[i] = put(reads[i], 1935 - len(ads[a]) + (i // 4) - 8, floorgen.edit(rng, ads[a], i % 2))
    renorm = Batch(o, reads)
    out["renorm"] = check(al, o, renorm, renorm.floors, "renormalisation in a window", "some")
    al.close()
    np.savez(sys.argv[1], **out)
    print("ROW_SKIP_TOP_CHILD_OK")


if __name__ == "__main__":
    sys.exit(main())
