"""The host reference of the glue kernels (tests/glue_ref.py) pinned without a GPU: its identities are Python's own
"%f" round trip, and the torch formulations in porechop_amd/pipeline.py (the route of aligners without the fused glue
kernels) agree with it on adversarial record sets."""
import math

import numpy as np
import pytest
import torch

from tests import glue_ref, gluegen
from tests.ref_pipeline import determine_barcode


def test_identities_are_the_printed_and_parsed_ratio_for_every_length_up_to_3000():
    from porechop_amd.pipeline import _identities
    for L in range(1, 3001):
        m = np.arange(L + 1)
        al = np.full(L + 1, L)
        want = [float("%f" % ((100.0 * k) / L)) for k in range(L + 1)]
        got = glue_ref.Fields().identities(list(zip(m.tolist(), al.tolist(), al.tolist())))
        assert [g[0] for g in got] == want, L
        assert [g[1] for g in got] == want, L
        rec = torch.zeros((L + 1, 8), dtype=torch.int32)
        rec[:, 5] = torch.from_numpy(m.astype(np.int32))
        rec[:, 6] = rec[:, 7] = L
        full, partial = _identities(rec)
        assert full.tolist() == want and partial.tolist() == want, L


def test_boundary_thresholds_separate_the_printed_from_the_unprinted_identity():
    """The data of the kernel tests: 1/3 prints 33.333333 < 100/3, 2/3 prints 66.666667 > 200/3 -- a comparison of the
    unrounded value lands on the other side of these thresholds."""
    thr = gluegen.boundary_thresholds()
    assert glue_ref.identity(1, 3) == 33.333333 and glue_ref.identity(2, 3) == 66.666667
    assert 100.0 / 3 in thr and 200.0 / 3 in thr and 33.333333 in thr and 66.666667 in thr
    flips = sum(1 for t in thr for m, L in gluegen.RATIOS if L and ((100.0 * m / L > t) != (glue_ref.identity(m, L) > t)))
    assert flips > 20


@pytest.mark.parametrize("seed", range(4))
def test_trimmed_interval_equals_python_slices(seed):
    from porechop_amd.pipeline import trimmed_interval
    rng = np.random.default_rng(seed)
    n = 4000
    length = rng.choice([0, 1, 2, 5, 150, 151, 300, 1000], size=n)
    st = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 1200, size=n))
    et = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 2500, size=n))
    et[::7] = length[::7] + rng.integers(1, 5, size=len(et[::7]))         # just past the length: the negative-index rule
    st[::11] = length[::11]
    s, e = trimmed_interval(torch.from_numpy(length.astype(np.int32)), torch.from_numpy(st.astype(np.int32)),
                            torch.from_numpy(et.astype(np.int32)))
    for i in range(n):
        ln = int(length[i])
        want = "x" * ln
        if st[i] or et[i]:
            want = want[int(st[i]):ln - int(et[i])]
        ws, wl = glue_ref.trimmed_interval(ln, int(st[i]), int(et[i]))
        assert wl == len(want)
        assert (int(s[i]), max(0, int(e[i]) - int(s[i]))) == (ws, wl), (ln, st[i], et[i])


def _scores(fields, bins):
    """The torch formulation's inputs: float64 [R, K] per side, NaN where the reference has no entry."""
    R, K = len(fields), len(bins)
    S = torch.full((R, K), math.nan, dtype=torch.float64)
    E = torch.full((R, K), math.nan, dtype=torch.float64)
    for r in range(R):
        for k, (sj, ej) in enumerate(bins):
            if sj >= 0 and fields[r][sj] is not None:
                S[r, k] = fields[r][sj][0]
            if ej >= 0 and fields[r][ej] is not None:
                E[r, k] = fields[r][ej][0]
    return S, E


def random_bins(rng, nbins, njobs, missing=0.2):
    return [(int(rng.integers(njobs)) if rng.random() > missing else -1, int(rng.integers(njobs)) if rng.random() > missing else -1)
            for _ in range(nbins)]


@pytest.mark.parametrize("nbins", [1, 2, 96])
@pytest.mark.parametrize("require_two", [False, True])
def test_call_barcodes_equals_the_reference(nbins, require_two):
    from porechop_amd.pipeline import call_barcodes
    rng = np.random.default_rng(nbins * 2 + require_two)
    R, J = 300, 24
    recs = gluegen.end_records(rng, R * J, 150, 50, zeros=False).reshape(J, R, 8)
    for r in range(0, R, 5):                          # the same bin best on both sides
        k = int(rng.integers(J))
        recs[k, r, 5] = recs[k, r, 7]
    fl = glue_ref.record_fields(recs.reshape(-1, 8), score_only_fails=True)
    untraced = rng.random((J, R)) < 0.1
    fields = [[None if untraced[j, r] else fl[j * R + r] for j in range(J)] for r in range(R)]
    bins = random_bins(rng, nbins, J)
    S, E = _scores(fields, bins)
    thresholds = [0.0, -1.0] + gluegen.boundary_thresholds()[::5]
    for thr in thresholds:
        for diff in (0.0, 5.0, 33.333333, 100.0 / 3):
            got = call_barcodes(nbins, S, E, thr, diff, require_two)
            want = [glue_ref.barcode_call(fields[r], bins, thr, diff, require_two) for r in range(R)]
            assert got.tolist() == want, (thr, diff)


def test_missing_entry_at_threshold_zero_is_absent_not_zero():
    """A read whose every barcode identity is 0.0, --barcode_threshold 0 --barcode_diff 0, bin 0 without a start entry
    and bin 1 with one: the reference calls bin 1 (the first PRESENT entry of its sorted lists); under
    --require_two_barcodes bin 0's missing side is ('none', 0.0) and the call is 'none'."""
    from porechop_amd.pipeline import call_barcodes
    assert determine_barcode({1: 0.0}, {0: 0.0, 1: 0.0}, 0.0, 0.0, False) == 1
    nan = math.nan
    S = torch.tensor([[nan, 0.0]], dtype=torch.float64)
    E = torch.tensor([[0.0, 0.0]], dtype=torch.float64)
    assert call_barcodes(2, S, E, 0.0, 0.0, False).tolist() == [1]
    # require_two: start side has only bin 1, end side has bins 0 and 1 (tied: bin 0 first) -> names differ -> 'none'
    assert determine_barcode({1: 0.0}, {0: 0.0, 1: 0.0}, 0.0, 0.0, True) == "none"
    assert call_barcodes(2, S, E, 0.0, 0.0, True).tolist() == [-1]
    # no start entry at all: ('none', 0.0) on that side
    S0 = torch.tensor([[nan, nan]], dtype=torch.float64)
    assert determine_barcode({}, {0: 0.0, 1: 0.0}, 0.0, 0.0, True) == "none"
    assert call_barcodes(2, S0, E, 0.0, 0.0, True).tolist() == [-1]
    assert call_barcodes(2, S0, E, -1.0, 0.0, False).tolist() == [0]
    assert call_barcodes(2, S0, S0, -1.0, 0.0, False).tolist() == [-1]
