"""Seeded synthetic record sets for the glue-kernel tests (TEST INFRASTRUCTURE; numpy only).

Records are built directly with consistent fields -- no DP: identities come from a small set of ratios whose six-decimal
values are not the ratios themselves (1/3 prints 33.333333, 2/3 66.666667), so thresholds can sit on, between and beside
the printed and the unprinted values."""
import math

import numpy as np

INT_MIN = -2147483648

# (matches, length): identities at and around rounding boundaries, ties between different ratios (1/3 = 2/6), 0 and 100
RATIOS = [(1, 3), (2, 3), (2, 6), (1, 6), (5, 6), (1, 7), (3, 7), (6, 7), (2, 9), (7, 9), (1, 11), (10, 11), (19, 21),
          (20, 23), (22, 24), (25, 28), (27, 33), (3, 3), (0, 4), (14, 15), (28, 29), (200, 201), (1, 2999)]


def printed(x):
    return float("%f" % x)


def boundary_thresholds(ratios=RATIOS):
    """Thresholds on a printed identity, one ulp either side of it, on the unprinted value and strictly between both."""
    out = set()
    for m, L in ratios:
        x = 100.0 * m / L
        r = printed(x)
        out.update([r, math.nextafter(r, math.inf), math.nextafter(r, -math.inf), x, (x + r) / 2])
    return sorted(out)


def end_records(rng, n, end_size, min_trim_size, zeros=True):
    """[n, 8] int32 end-window records: -1 (failed), -2 (score only), all-zero (not computed, when `zeros`) and traced
    records whose spans end at the window's edges and straddle min_trim_size."""
    recs = np.zeros((n, 8), dtype=np.int32)
    kind = rng.choice(4, size=n, p=[0.08, 0.08, 0.05 if zeros else 0.0, 0.79 if zeros else 0.84])
    ratios = np.array(RATIOS, dtype=np.int64)[rng.integers(len(RATIOS), size=n)]
    m, fl = ratios[:, 0], ratios[:, 1]
    al = np.where(rng.random(n) < 0.6, fl, np.maximum(m, 1) + (rng.random(n) * (fl + 12 - np.maximum(m, 1))).astype(np.int64))
    span = np.array([min_trim_size - 1, min_trim_size, min_trim_size + 1, 1, 0])[rng.integers(5, size=n)]
    span = np.where(span == 0, rng.integers(1, end_size + 1, size=n), span).clip(1, end_size)
    w = rng.random(n)
    rs = np.where(w < 0.25, 0, np.where(w < 0.5, end_size - span, (rng.random(n) * (end_size - span + 1)).astype(np.int64)))
    ok = np.stack([rs, rs + span - 1, np.zeros(n, np.int64), fl - 1, 3 * m, m, al, fl], axis=1)
    failed = np.zeros((n, 8), dtype=np.int64) - 1
    failed[:, 4] = np.where(rng.random(n) < 0.5, INT_MIN, rng.integers(-50, 50, size=n))
    failed[:, 5:] = np.where(rng.random((n, 1)) < 0.5, 0, 20)        # junk fields behind the failure marker: must not matter
    score = np.stack([np.full(n, -2), rng.integers(0, end_size, size=n), rng.integers(0, 24, size=n), np.full(n, 23),
                      rng.integers(-20, 80, size=n), np.full(n, 24), np.full(n, 24), np.full(n, 24)], axis=1)
    recs[kind == 0] = failed[kind == 0]
    recs[kind == 1] = score[kind == 1]
    recs[kind == 3] = ok[kind == 3]
    return recs


def traced_mask(rng, jobs, n, p=0.75):
    """[jobs, (n + 63) // 64] int64: random bits, bit 63 / bit 0 of many words cleared, no bit at or beyond n."""
    words = (n + 63) // 64
    bits = rng.random((jobs, words * 64)) < p
    ends = rng.random((jobs, words)) < 0.5
    bits[:, 63::64] &= ~ends
    bits[:, 0::64] &= rng.random((jobs, words)) < 0.7
    bits[:, n:] = False
    return pack_bits(bits)


def pack_bits(bits):
    """bool [J, words * 64] -> int64 [J, words], bit r % 64 of word r // 64."""
    J, nb = bits.shape
    w = bits.reshape(J, nb // 64, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(w, axis=2).view(np.int64)


def unpack_bits(mask, n):
    m = np.ascontiguousarray(mask).view(np.uint64)
    return ((m[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(m.shape[0], -1)[:, :n]
