"""The rule behind the score floor of the middle scan's second pass, on the oracle alone (no GPU).

Pipeline.identity_score_bound(m, threshold) claims: an alignment of an m-base adapter whose full-adapter identity reaches
`threshold` has a raw score of at least the bound.  The library leaves a pair untraced when its best score is below the
bound (pc_scan_device_floored), so the claim is what makes the floored scan exact.  No earlier test asserts it directly
(tests/test_phase_a_pruning.py only checks when a bound exists): here it is checked on a few thousand seeded windows with
planted, edited adapter copies, for every adapter length of the panel and the thresholds 75 / 85 / 90."""
import random

import numpy as np

from tests import floorgen
from tests.golden_io import load_panel

THRESHOLDS = (75.0, 85.0, 90.0)
PER_LENGTH = 320


def panel_adapters_by_length():
    """One panel sequence per distinct length (the middle scan takes the start and end sequences of the matching sets)."""
    by_len = {}
    for a in load_panel():
        for side in (a["start"], a["end"]):
            if side:
                by_len.setdefault(len(side[1]), side[1])
    return by_len


def test_identity_at_threshold_implies_score_at_bound(oracle):
    by_len = panel_adapters_by_length()
    assert {22, 28, 30, 33} <= set(by_len)                    # the headline's four middle adapters among them
    rng = random.Random(20261)
    reached = {t: 0 for t in THRESHOLDS}
    total = 0
    for m, ad in sorted(by_len.items()):
        windows = []
        for _ in range(PER_LENGTH):
            copy = floorgen.edit(rng, ad, rng.randint(0, 8))
            if rng.random() < 0.25:                            # truncated copies: high identity over a short span is not a hit
                copy = copy[rng.randint(0, len(copy) // 2):]
            body = floorgen.random_bases(rng, rng.randint(120, 400))
            pos = rng.randint(0, len(body))
            windows.append(body[:pos] + copy + body[pos:])
        lens = np.array([len(w) for w in windows], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
        arena = np.frombuffer("".join(windows).encode(), dtype=np.uint8)
        n = len(windows)
        o = oracle.align_many(arena, offs, lens, np.frombuffer(ad.encode(), dtype=np.uint8), np.zeros(n, dtype=np.int64),
                              np.full(n, m, dtype=np.int32), floorgen.SCORES)
        total += n
        for rec in o:
            if rec[0] == -1 or rec[8] == 0:
                continue
            full = round(100.0 * float(rec[7]) / float(rec[8]), 6)
            for t in THRESHOLDS:
                bound = floorgen.score_bound(m, t)
                assert bound is not None and bound > 0
                if full >= t:
                    reached[t] += 1
                    assert rec[4] >= bound, (m, t, full, int(rec[4]), bound)
    assert total >= 3000
    assert all(reached[t] >= 200 for t in THRESHOLDS), reached          # the implication was not checked on nothing


def test_batches_hold_both_sides_of_the_comparison(oracle):
    """The batches of tests/test_gpu_pass2_floor.py: pairs whose best score equals the bound exactly and the bound minus one
    are present, identities straddle the threshold, and some pairs above the bound are still not hits (the floor is a
    necessary condition, not the decision)."""
    for seed, ragged in ((11, False), (12, True)):
        b = floorgen.Batch(oracle, seed, ragged)
        at = [(a, s) for a, s, want in b.exact if want == b.bounds[a]]
        under = [(a, s) for a, s, want in b.exact if want == b.bounds[a] - 1]
        assert len(at) == 3 and len(under) == 3
        below = b.below(b.bounds)
        for a, s in at:
            assert not below[a, s]
        for a, s in under:
            assert below[a, s]
        hit = b.full >= b.threshold
        assert hit.sum() >= 20 and (~hit & ~below).sum() >= 5
        assert not (hit & below).any()                         # the proof, on this batch
        assert 0.5 < below.mean() < 0.98
        if ragged:
            assert b.lens.min() == 300 and b.lens.max() == 2000
        f = floorgen.lane63_floors(b)
        assert b.below(f).sum() == b.score.size - 1 and not b.below(f)[0, 63]
