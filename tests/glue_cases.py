"""TEST INFRASTRUCTURE: the case bodies of the middle scan's glue checks, against the plain host reference (tests/glue_ref.py).

Each takes the glue object -- the Aligner (tests/test_gpu_glue_kernels.py) or the torch glue (tests/test_middle_glue_cpu.py);
both keep one contract, porechop_amd/middle.py -- a function `dev` that puts a numpy array where the glue wants its tensors,
and `sync`, called after every glue step (the Aligner's sync)."""
import math
import random

import numpy as np

from tests import glue_ref, gluegen

SIZES = [1, 63, 64, 65, 255, 256, 257, 4097]
STAT_BIG = glue_ref.STAT_BIG


def _nothing():
    pass


def trim_inputs(rng, n):
    length = rng.choice([0, 1, 2, 7, 150, 151, 300, 1000, 5000], size=n).astype(np.int32)
    st = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 1200, size=n)).astype(np.int32)
    et = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 2500, size=n)).astype(np.int32)
    k = rng.random(n)
    et = np.where(k < 0.1, length + rng.integers(1, 40, size=n), et).astype(np.int32)       # past the length: negative index
    st = np.where((k >= 0.1) & (k < 0.15), length + rng.integers(0, 3, size=n), st).astype(np.int32)   # start past the end
    off = np.cumsum(np.concatenate([[5], length[:-1].astype(np.int64) + 3])).astype(np.int64)
    return off, length, st, et


def check_trim_windows(glue, dev, off, length, st, et, sync=_nothing):
    toff, tlen, stats = glue.trim_windows(dev(off), dev(length), dev(st), dev(et))
    sync()
    toff, tlen = toff.cpu().numpy(), tlen.cpu().numpy()
    want = [glue_ref.trimmed_interval(int(length[i]), int(st[i]), int(et[i])) for i in range(len(off))]
    ws = np.array([w[0] for w in want], dtype=np.int64)
    wl = np.array([w[1] for w in want], dtype=np.int64)
    assert np.array_equal(tlen, wl)
    assert np.array_equal(toff, off + ws)
    assert stats.cpu().tolist() == glue_ref.trim_stats(wl.tolist())


def trim_windows_equal_python_slices(glue, dev, n, sync=_nothing):
    off, length, st, et = trim_inputs(np.random.default_rng(n), n)
    check_trim_windows(glue, dev, off, length, st, et, sync)


def trim_windows_edges(glue, dev, sync=_nothing):
    rng = np.random.default_rng(3)
    off, length, st, et = trim_inputs(rng, 4097)
    st[:300] = 0
    et[:300] = 0                                     # both trims 0: the whole read
    check_trim_windows(glue, dev, off, length, st, et, sync)
    for n in (1, 257, 4097):                          # all-empty batches: "shortest non-empty" stays "none" (0)
        z = np.zeros(n, dtype=np.int32)
        check_trim_windows(glue, dev, np.arange(n, dtype=np.int64), z, z + 1, z, sync)
        L = np.full(n, 10, dtype=np.int32)
        check_trim_windows(glue, dev, np.arange(n, dtype=np.int64), L, L, z + 3, sync)
    e = np.zeros(0, dtype=np.int32)
    check_trim_windows(glue, dev, np.zeros(0, dtype=np.int64), e, e, e, sync)


def middle_records(rng, n):
    recs = gluegen.end_records(rng, n, 5000, 1)
    return recs


def middle_hits_equal_the_reference(glue, dev, n, sync=_nothing):
    rng = np.random.default_rng(n + 1)
    recs = middle_records(rng, n)
    F = glue_ref.record_fields(recs)
    thrs = [90.0, 66.666667, 200.0 / 3, math.nextafter(66.666667, 100), 33.333333, 100.0 / 3] if n < 1_000_000 else [100.0 / 3]
    t = dev(recs)
    for thr in thrs:
        full, hit = glue.middle_hits(t, thr)
        sync()
        wf, wh = zip(*[glue_ref.middle_hit(f, thr) for f in F])
        assert np.array_equal(full.cpu().numpy(), np.nan_to_num(np.array(wf), nan=0.0)), thr
        assert hit.cpu().numpy().tolist() == list(wh), thr


def middle_hits_keep_the_batch_shape_and_accept_an_empty_batch(glue, dev, sync=_nothing):
    rng = np.random.default_rng(2)
    recs = middle_records(rng, 3 * 65).reshape(3, 65, 8)
    full, hit = glue.middle_hits(dev(recs), 33.333333)
    sync()
    assert tuple(full.shape) == (3, 65) and tuple(hit.shape) == (3, 65)
    F = glue_ref.record_fields(recs.reshape(-1, 8))
    assert hit.cpu().numpy().reshape(-1).tolist() == [glue_ref.middle_hit(f, 33.333333)[1] for f in F]
    full, hit = glue.middle_hits(dev(np.zeros((0, 8), dtype=np.int32)), 90.0)
    sync()
    assert full.numel() == 0 and hit.numel() == 0


def round_consume_equals_one_round_of_find_middle_adapters(glue, dev, n, A, sync=_nothing):
    rng = np.random.default_rng(n * 100 + A)
    Dn = n + 5                                                   # act: a strict subset of the dirty reads
    recs = middle_records(rng, A * Dn).reshape(A, Dn, 8)
    thr = [90.0, 66.666667, 200.0 / 3, 33.333333][(n + A) % 4]
    F = glue_ref.record_fields(recs.reshape(-1, 8))
    full_all = np.nan_to_num(np.array([f[0] for f in F]), nan=0.0).reshape(A, Dn)
    failed = recs[:, :, 0] == -1
    full_all[failed & (rng.random((A, Dn)) < 0.5)] = 100.0          # -1 records whose `full` is at or above the threshold
    full_all[failed & (rng.random((A, Dn)) < 0.3)] = thr
    cur = rng.integers(0, A + 1, size=Dn).astype(np.int64)           # cur == A: nothing left to consume
    last = rng.random(Dn) < 0.2                                      # a hit at the last adapter only
    recs[:, last, 0] = -1
    recs[A - 1, last] = [3, 40, 0, 9, 30, 10, 10, 10]
    full_all[:, last] = 0.0
    full_all[A - 1, last] = 100.0
    cur[last] = np.minimum(cur[last], A - 1)
    act = np.sort(rng.choice(Dn, size=n, replace=False)).astype(np.int64)
    rng.shuffle(act)
    anyh, a_hit, cnt, stats = glue.round_consume(dev(full_all), dev(recs), dev(cur), dev(act), thr)
    sync()
    want_h, want_a, want_c, used, amin = [], [], [], 0, None
    for d in act.tolist():
        a, m, u = glue_ref.consume(full_all[:, d].tolist(), recs[:, d, 0].tolist(), (recs[:, d, 1] + 1).tolist(), int(cur[d]), thr)
        want_h.append(a is not None)
        want_a.append(0 if a is None else a)
        want_c.append(m)
        used += u
        if a is not None:
            amin = a if amin is None else min(amin, a)
    assert anyh.cpu().tolist() == want_h
    assert a_hit.cpu().tolist() == want_a
    assert cnt.cpu().tolist() == want_c
    assert stats.cpu().tolist() == [used, sum(want_h), 0 if amin is None else STAT_BIG - amin, sum(want_c)]
    anyh, a_hit, cnt, stats = glue.round_consume(dev(full_all), dev(recs), dev(cur), dev(np.zeros(0, dtype=np.int64)), thr)
    sync()
    assert anyh.numel() == 0 and stats.cpu().tolist() == [0, 0, 0, 0]


def group_survivors_equal_the_masked_any(glue, dev, n, words, sync=_nothing):
    rng = np.random.default_rng(n * 7 + words)
    G = 5
    mask = np.where(rng.random((n, words)) < 0.6, 0, rng.integers(-2**31, 2**31, size=(n, words))).astype(np.int32)
    mask[::9, -1] = np.int32(-2**31)                             # bit 31 alone
    gm = rng.integers(-2**31, 2**31, size=(G, words)).astype(np.int32)
    gm[0] = 0
    gm[1, :] = 0
    gm[1, -1] = np.int32(-2**31)                                 # bit 31 set: a negative int32, as pipeline.py builds it
    gm[2] = np.int32(1)
    cand, counts = glue.group_survivors(dev(mask), dev(gm))
    sync()
    want = np.array([[any(int(mask[w, k]) & int(gm[g, k]) for k in range(words)) for w in range(n)] for g in range(G)],
                    dtype=bool).reshape(G, n)
    assert np.array_equal(cand.cpu().numpy(), want)
    assert counts.cpu().tolist() == want.sum(axis=1).tolist()
    assert want[1].any() or n < 9


# ---- round_consume_select: the case shapes of select_case in tests/mask_rule_child.py --------------------------------------
SELECT_CASES = [(floored, nact, S) for floored in (False, True) for nact, S in ((1, 1), (255, 1), (256, 1), (257, 1), (1, 98), (257, 98))]


def round_consume_select_equals_the_headers_rule(glue, dev, floored, nact, S, sync=_nothing):
    """need and the per-set counts against pcm::must_realign as the library compiles it for the host
    (batch.mask_rule_must_realign).  Every active read stands at adapter 0 and has at most one record at the threshold, so the
    consuming half finds exactly the hit the case chose."""
    from porechop_amd.batch import mask_rule_must_realign
    rng = random.Random(77 + 1000 * nact + 10 * S + floored)
    A = 2 * S if S > 1 else 3
    Dn = nact + 5
    set_of = np.array([min(a // 2, S - 1) for a in range(A)], dtype=np.int32)
    act = np.array(rng.sample(range(Dn), nact), dtype=np.int64)
    anyh = np.array([rng.random() < 0.8 for _ in range(nact)], dtype=bool)
    a_hit = np.array([rng.randrange(A) for _ in range(nact)], dtype=np.int32)
    rec = np.zeros((A, Dn, 8), dtype=np.int32)
    rec[:, :, 2:] = 7
    full = np.zeros((A, Dn), dtype=np.float64)
    for k in range(nact):
        d, h = int(act[k]), int(a_hit[k])
        hs = rng.randrange(0, 900)
        he = hs + rng.choice((-1, 0, 1, 20, 33))                 # inclusive end; -1: a hit interval of length 0
        for a in range(A):
            kind = rng.randrange(8)
            if kind == 0:
                r0, r1 = -1, 0
            elif kind == 1:                                      # meets the mask's left edge by 0 or 1 columns
                r1 = hs - rng.choice((0, 1)); r0 = r1 - rng.randrange(0, 30)
            elif kind == 2:                                      # ... its right edge
                r0 = he + 1 - rng.choice((0, 1)); r1 = r0 + rng.randrange(0, 30)
            elif kind == 3:
                r0 = rng.randrange(0, 1000); r1 = r0 - rng.randrange(1, 5)       # an odd record
            else:
                r0 = rng.randrange(0, 1000); r1 = r0 + rng.randrange(0, 40)
            rec[a, d, 0], rec[a, d, 1] = r0, r1
        rec[h, d, 0], rec[h, d, 1] = hs, he
        if anyh[k]:
            full[h, d] = 100.0
    cur = np.zeros(Dn, dtype=np.int64)
    got_h, got_a, cnt, stats, need = glue.round_consume_select(dev(full), dev(rec), dev(cur), dev(act), 90.0, dev(set_of), S, floored)
    sync()
    assert got_h.cpu().tolist() == anyh.tolist()
    assert [a for a, h in zip(got_a.cpu().tolist(), anyh) if h] == [int(a) for a, h in zip(a_hit, anyh) if h]
    want = np.zeros((S, nact), dtype=np.uint8)
    for k in range(nact):
        if not anyh[k]:
            continue
        d, h = int(act[k]), int(a_hit[k])
        rs, re = int(rec[h, d, 0]), int(rec[h, d, 1]) + 1
        for a in range(h, A):
            if mask_rule_must_realign(a, h, rec[a, d, 0], rec[a, d, 1], rs, re, floored):
                want[set_of[a], k] = 1
    got = need.cpu().numpy().astype(np.uint8)
    assert got.shape == want.shape and (got == want).all(), ("need", nact, S, floored, int((got != want).sum()))
    stats = stats.cpu().tolist()
    assert len(stats) == 4 + S and stats[4:] == want.sum(axis=1).tolist(), ("counts", nact, S, floored)
    hits = [int(a) for a, h in zip(a_hit, anyh) if h]
    assert stats[1] == len(hits) and stats[2] == (STAT_BIG - min(hits) if hits else 0)
    assert stats[3] == sum(max(0, int(rec[a_hit[k], act[k], 1]) + 1 - int(rec[a_hit[k], act[k], 0])) for k in range(nact) if anyh[k])
    assert 0 < want.sum() < want.size or nact == 1
