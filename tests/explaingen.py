"""Seeded record tables for the explain tests (TEST INFRASTRUCTURE; numpy only): the records of tests/gluegen.py laid
out as J jobs over n reads, with what pc_phase_b_explain has to get right constructed ON PURPOSE --
  tied trims        a second job of the same side carries a copy of the first one's record for every fourth read,
                    so two alignments justify the same (often the largest) trim and the deciding job is the earlier one
  tied scores       the entries of two bins of one side carry the same (matches, full_len) for every third read, and
                    1/3 = 2/6 ties between different ratios come from gluegen.RATIOS
  absent bins       bins without a start or an end entry (-1), also as the first bin
  shared jobs       optionally one job serves two bins of a side (the job -> bin table has no inverse then)."""
import numpy as np

from tests import gluegen


def case(rng, n, J, nbins, shared_jobs=False, end_size=150, min_trim_size=50):
    """-> (records int32 [*, 8], job offsets int64 [J], sides int32 [J], bins [(start job or -1, end job or -1)])."""
    sides = rng.integers(0, 2, size=J).astype(np.int32)
    if J >= 4:
        sides[:4] = [0, 1, 0, 1]
    offs = np.zeros(J, dtype=np.int64)
    pos = 0
    for j in rng.permutation(J):                          # shuffled, gapped layout: job order is not record order
        offs[j] = pos
        pos += n + 3
    recs = np.zeros((pos, 8), dtype=np.int32)
    recs[:] = [-1, -1, -1, -1, 0, 0, 0, 0]
    for j in range(J):
        recs[offs[j]:offs[j] + n] = gluegen.end_records(rng, n, end_size, min_trim_size, zeros=False)
    rows = np.arange(n)
    for side in (0, 1):                                   # tied trims
        js = np.nonzero(sides == side)[0]
        if js.size >= 2:
            a, b = js[0], js[-1]
            recs[offs[b] + rows[::4]] = recs[offs[a] + rows[::4]]
    bins = []
    if nbins:
        if shared_jobs or J < 2 * nbins:
            pick = lambda: int(rng.integers(J)) if rng.random() > 0.2 else -1
            bins = [(pick(), pick()) for _ in range(nbins)]
        else:                                             # every job the entry of at most one bin per side
            perm_s, perm_e = rng.permutation(J), rng.permutation(J)
            bins = [(int(perm_s[k]) if rng.random() > 0.2 else -1, int(perm_e[k]) if rng.random() > 0.2 else -1) for k in range(nbins)]
        if nbins >= 2:
            bins[0] = (-1, bins[0][1])                    # a bin without a start entry before one with
        for which in (0, 1):                              # tied scores between two bins of a side
            js = [b[which] for b in bins if b[which] >= 0]
            if len(js) >= 2 and js[0] != js[-1]:
                src, dst = recs[offs[js[0]] + rows[::3]], recs[offs[js[-1]] + rows[::3]]
                both = (src[:, 0] >= 0) & (dst[:, 0] >= 0)
                dst[both, 5], dst[both, 7] = src[both, 5], src[both, 7]
                dst[both, 6] = np.maximum(dst[both, 6], dst[both, 5])
                recs[offs[js[-1]] + rows[::3]] = dst
    return recs, offs, sides, bins
