"""The per-read glue kernels on the MI355X, element by element against the plain host reference (tests/glue_ref.py):
the phase-B reduction (trims and barcode calls, with and without a traced mask), the middle scan's trimmed windows,
hits, consuming rounds and prefilter survivors, and the index plumbing of the pruned phase B.  Synthetic records with
consistent fields (tests/gluegen.py), thresholds on and beside rounding boundaries, batch sizes across the wave, the
block and the 64-read mask word."""
import math

import numpy as np
import pytest

from tests import glue_cases, glue_ref, gluegen
from tests.glue_cases import SIZES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    a = porechop_amd.Aligner(["ACGTACGTAC"])
    yield a
    a.close()


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- phase B: pc_phase_b_reduce ----------------------------------------------------------------------------------------
def reduce_case(rng, n, J, nbins, end_size=150, min_trim_size=50):
    """J jobs of n reads laid out at shuffled, gapped offsets; all-zero records only in jobs no bin uses."""
    bins = [(int(rng.integers(J)) if rng.random() > 0.2 else -1, int(rng.integers(J)) if rng.random() > 0.2 else -1)
            for _ in range(nbins)]
    if nbins >= 2:
        bins[0] = (-1, bins[0][1] if bins[0][1] >= 0 else 0)          # a bin without a start entry before one with
        bins[1] = (bins[1][0] if bins[1][0] >= 0 else 0, bins[1][1])
    used = {j for b in bins for j in b if j >= 0}
    order = rng.permutation(J)
    gap = 3
    offs = np.zeros(J, dtype=np.int64)
    pos = 0
    for j in order:
        offs[j] = pos
        pos += n + gap
    recs = np.zeros((pos, 8), dtype=np.int32)
    recs[:] = [-1, -1, -1, -1, 0, 0, 0, 0]
    for j in range(J):
        recs[offs[j]:offs[j] + n] = gluegen.end_records(rng, n, end_size, min_trim_size, zeros=j not in used)
    for r in range(0, n, 4):                              # the same bin best on both sides, ties at the maximum
        if bins:
            sj, ej = bins[int(rng.integers(len(bins)))]
            for j in (sj, ej):
                if j >= 0 and recs[offs[j] + r, 0] >= 0:
                    recs[offs[j] + r, 5] = recs[offs[j] + r, 7]
    sides = rng.integers(0, 2, size=J).astype(np.int32)
    return recs, offs, sides, bins


def host_reduce(recs, offs, sides, bins, n, mask_bits, p, thr, diff, two):
    F = glue_ref.record_fields(recs, score_only_fails=True)
    J = len(sides)
    st, et, call = [], [], []
    for r in range(n):
        fields = [F[offs[j] + r] if mask_bits is None or mask_bits[j, r] else None for j in range(J)]
        a, b = glue_ref.end_trims(fields, sides, *p)
        st.append(a)
        et.append(b)
        if bins:
            call.append(glue_ref.barcode_call(fields, bins, thr, diff, two))
    return st, et, call


def run_reduce(al, recs, offs, sides, bins, n, p, thr, diff, two, mask=None):
    import torch
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    et = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    call = torch.full((n,), -7, dtype=torch.int32, device="cuda") if bins else None
    al.phase_b_reduce(dev(recs), n, offs, sides, *p, st, et, bins=bins or None, barcode_threshold=thr, barcode_diff=diff,
                      require_two=two, call=call, traced_mask=None if mask is None else dev(mask))
    al.sync()
    return st.cpu().tolist(), et.cpu().tolist(), (call.cpu().tolist() if bins else [])


END_THR = [75.0, 33.333333, 100.0 / 3, math.nextafter(33.333333, 0), math.nextafter(33.333333, 100),
           66.666667, 200.0 / 3, (200.0 / 3 + 66.666667) / 2, 0.0]
BC = [(0.0, 0.0), (-1.0, 0.0), (33.333333, 0.0), (100.0 / 3, 33.333333), (66.666667, 100.0 / 3 - 33.333333),
      (75.0, 5.0), (math.nextafter(66.666667, 0), 66.666667 - 33.333333), (0.0, 33.333334 - 1e-9)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("masked", [False, True])
def test_phase_b_reduce_equals_the_reference(al, n, masked):
    rng = np.random.default_rng(n * 2 + masked)
    shapes = [(1, 0), (3, 1), (7, 2), (24, 2)] + ([(196, 96)] if n >= 255 else [(40, 96)])
    for J, nbins in shapes:
        recs, offs, sides, bins = reduce_case(rng, n, J, nbins)
        mask = gluegen.traced_mask(rng, J, n) if masked else None
        bits = gluegen.unpack_bits(mask, n) if masked else None
        for k in range(2 if J < 196 else 1):
            et_thr = END_THR[int(rng.integers(len(END_THR)))] if k else END_THR[(n + J) % len(END_THR)]
            p = (150, 50 if k else 51, 0 if k else 7, et_thr)
            thr, diff = BC[(J + k + n) % len(BC)]
            two = bool((k + J + nbins) % 2)
            want = host_reduce(recs, offs, sides, bins, n, bits, p, thr, diff, two)
            got = run_reduce(al, recs, offs, sides, bins, n, p, thr, diff, two, mask)
            for name, g, w in zip(("start_trim", "end_trim", "call"), got, want):
                bad = [i for i in range(len(w)) if g[i] != w[i]]
                assert not bad, (name, J, nbins, p, thr, diff, two, bad[:5], [(g[i], w[i]) for i in bad[:5]])


def test_phase_b_reduce_every_threshold_and_diff_on_a_boundary(al):
    """One batch, every boundary threshold as end_threshold and as barcode_threshold, diffs whose second + diff rounds."""
    rng = np.random.default_rng(11)
    n, J, nbins = 257, 12, 5
    recs, offs, sides, bins = reduce_case(rng, n, J, nbins)
    F = glue_ref.record_fields(recs, score_only_fails=True)
    fields = [[F[offs[j] + r] for j in range(J)] for r in range(n)]
    thrs = gluegen.boundary_thresholds()
    for t in thrs:
        p = (150, 50, 3, t)
        st, et, _ = run_reduce(al, recs, offs, sides, [], n, p, 0.0, 0.0, False)
        want = [glue_ref.end_trims(fields[r], sides, *p) for r in range(n)]
        assert list(zip(st, et)) == want, t
    for t in thrs[::3] + [0.0, -1.0]:
        for diff in (0.0, 100.0 / 3 - 33.333333, 33.333333, 200.0 / 3 - 100.0 / 3, math.nextafter(0.0, 1.0)):
            for two in (False, True):
                _, _, call = run_reduce(al, recs, offs, sides, bins, n, (150, 50, 0, 75.0), t, diff, two)
                want = [glue_ref.barcode_call(fields[r], bins, t, diff, two) for r in range(n)]
                assert call == want, (t, diff, two)


def test_phase_b_reduce_missing_entry_at_threshold_zero(al):
    """--barcode_threshold 0 --barcode_diff 0, every identity 0.0, bin 0 without a start entry, bin 1 with one: the
    reference calls bin 1 (the first present entry of its sorted lists), and 'none' under --require_two_barcodes."""
    zero = [0, 10, 0, 9, -30, 0, 12, 12]                # a traced alignment with 0 matches: identity 0.0
    recs = np.array([zero, zero, zero], dtype=np.int32)
    offs, sides = [0, 1, 2], [0, 1, 1]
    bins = [(-1, 1), (0, 2)]
    assert run_reduce(al, recs, offs, sides, bins, 1, (150, 50, 0, 75.0), 0.0, 0.0, False)[2] == [1]
    assert run_reduce(al, recs, offs, sides, bins, 1, (150, 50, 0, 75.0), 0.0, 0.0, True)[2] == [-1]
    assert run_reduce(al, recs, offs, sides, [(-1, -1)], 1, (150, 50, 0, 75.0), -1.0, 0.0, False)[2] == [-1]
    assert run_reduce(al, recs, offs, sides, [(-1, 1)], 1, (150, 50, 0, 75.0), 0.0, 0.0, True)[2] == [-1]


def test_phase_b_reduce_large_batch(al):
    rng = np.random.default_rng(5)
    n, J = 100_003, 3
    recs, offs, sides, bins = reduce_case(rng, n, J, 2)
    mask = gluegen.traced_mask(rng, J, n)
    p = (150, 50, 2, 100.0 / 3)
    for m in (None, mask):
        want = host_reduce(recs, offs, sides, bins, n, None if m is None else gluegen.unpack_bits(m, n), p, 33.333333, 0.0, False)
        got = run_reduce(al, recs, offs, sides, bins, n, p, 33.333333, 0.0, False, m)
        assert got == tuple(want)


def test_phase_b_reduce_empty_batch(al):
    import torch
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    al.phase_b_reduce(torch.zeros((4, 8), dtype=torch.int32, device="cuda"), 0, [0], [0], 150, 50, 0, 75.0, e, e)
    al.sync()


# ---- the middle scan's glue (pc_middle.hip) ------------------------------------------------------------------------------
# (the case bodies are tests/glue_cases.py's: tests/test_middle_glue_cpu.py holds the torch glue to the same ones)
@pytest.mark.parametrize("n", SIZES + [1_000_003])
def test_trim_windows_equals_python_slices(al, n):
    glue_cases.trim_windows_equal_python_slices(al, dev, n, al.sync)


def test_trim_windows_edges(al):
    glue_cases.trim_windows_edges(al, dev, al.sync)


@pytest.mark.parametrize("n", SIZES + [1_000_003])
def test_middle_hits_equal_the_reference(al, n):
    glue_cases.middle_hits_equal_the_reference(al, dev, n, al.sync)


def test_middle_hits_keep_the_batch_shape_and_accept_an_empty_batch(al):
    glue_cases.middle_hits_keep_the_batch_shape_and_accept_an_empty_batch(al, dev, al.sync)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("A", [1, 2, 7, 33])
def test_round_consume_equals_one_round_of_find_middle_adapters(al, n, A):
    glue_cases.round_consume_equals_one_round_of_find_middle_adapters(al, dev, n, A, al.sync)


@pytest.mark.parametrize("n", SIZES + [0])
@pytest.mark.parametrize("words", [1, 3])
def test_group_survivors_equal_the_masked_any(al, n, words):
    glue_cases.group_survivors_equal_the_masked_any(al, dev, n, words, al.sync)


# ---- the index plumbing of the pruned phase B (pc_select.hip) -----------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [1_000_003])
def test_gather_records_with_duplicate_and_unsorted_indices(al, n):
    rng = np.random.default_rng(n + 3)
    N = max(1, n // 3 + 1)
    recs = rng.integers(-2**31, 2**31, size=(N, 8)).astype(np.int32)
    idx = rng.integers(0, N, size=n).astype(np.int64)
    idx[: min(n, 5)] = N - 1
    out = al.gather_records(dev(recs), dev(idx))
    al.sync()
    assert np.array_equal(out.cpu().numpy(), recs[idx])
    import torch
    out = al.gather_records(dev(recs), torch.zeros(0, dtype=torch.int64, device="cuda"))
    al.sync()
    assert out.shape[0] == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("J", [1, 3, 196])
def test_phase_b_gather_lists_every_selected_pair_once(al, n, J):
    import torch
    rng = np.random.default_rng(n * 1000 + J)
    bits = rng.random((J, ((n + 63) // 64) * 64)) < rng.choice([0.02, 0.5, 1.0], size=(J, 1))
    bits[:, n:] = False
    if J > 1:
        bits[1] = False                                              # a job with nothing selected
    mask = gluegen.pack_bits(bits)
    cnt = bits.sum(axis=1)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    T = int(cnt.sum())
    job_off = (rng.permutation(J) * (n + 2)).astype(np.int64)
    side = rng.integers(0, 2, size=J).astype(np.int32)
    so = rng.integers(0, 10**9, size=n).astype(np.int64)
    sl = rng.integers(0, 150, size=n).astype(np.int32)
    eo = rng.integers(0, 10**9, size=n).astype(np.int64)
    el = rng.integers(0, 150, size=n).astype(np.int32)
    cursor = dev(np.full(J, 12345, dtype=np.int64))
    # (one spare slot: the outputs are never empty tensors, whose null pointers the entry point refuses; it stays -1)
    win_off = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
    win_len = torch.full((T + 1,), -1, dtype=torch.int32, device="cuda")
    dest = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
    pjob = torch.full((T + 1,), -1, dtype=torch.int32, device="cuda")
    pread = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
    al.phase_b_gather(dev(mask), n, dev(first), cursor, dev(job_off), dev(side), dev(so), dev(sl), dev(eo), dev(el),
                      win_off, win_len, dest, pjob, pread)
    al.sync()
    assert cursor.cpu().tolist() == cnt.tolist()
    wo, wl, de, pj, pr = (t.cpu().numpy() for t in (win_off, win_len, dest, pjob, pread))
    assert (wo[T], wl[T], de[T], pj[T], pr[T]) == (-1, -1, -1, -1, -1)
    for j in range(J):
        lo, hi = int(first[j]), int(first[j] + cnt[j])
        reads = np.nonzero(bits[j, :n])[0]
        assert sorted(pr[lo:hi].tolist()) == reads.tolist(), j          # which block claims the cursor first is free
        assert (pj[lo:hi] == j).all()
        assert np.array_equal(de[lo:hi], job_off[j] + pr[lo:hi])
        o, L = (eo, el) if side[j] else (so, sl)
        assert np.array_equal(wo[lo:hi], o[pr[lo:hi]]) and np.array_equal(wl[lo:hi], L[pr[lo:hi]])


@pytest.mark.parametrize("n", SIZES)
def test_phase_b_scatter_writes_records_and_keeps_the_best_barcode_identity(al, n):
    import torch
    rng = np.random.default_rng(n + 17)
    J = 5
    records = gluegen.end_records(rng, J * n, 150, 50).reshape(J * n, 8)
    before = records.copy()
    count = max(1, (J * n) // 2)
    dest = rng.choice(J * n, size=count, replace=False).astype(np.int64)
    pjob = (dest // n).astype(np.int32)
    pread = (dest % n).astype(np.int64)
    traced = gluegen.end_records(rng, count, 150, 50)
    traced[::3, 5] = traced[::3, 7]
    side = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    calls = np.array([1, 1, 0, 1, 0], dtype=np.int32)
    best0 = np.where(rng.random((2, n)) < 0.3, [glue_ref.identity(2, 3)], 0.0)
    rec_t, best_t = dev(records), dev(best0)
    al.phase_b_scatter(dev(traced), dev(dest), dev(pjob), dev(pread), rec_t, dev(side), dev(calls), best_t, n)
    al.sync()
    want = before.copy()
    want[dest] = traced
    assert np.array_equal(rec_t.cpu().numpy(), want)
    wb = best0.copy()
    F = glue_ref.record_fields(traced)
    for k in range(count):
        j = int(pjob[k])
        if calls[j] and traced[k, 0] != -1 and traced[k, 7] > 0:
            wb[side[j], pread[k]] = max(wb[side[j], pread[k]], F[k][0])
    assert np.array_equal(best_t.cpu().numpy(), wb)
    al.phase_b_scatter(dev(traced[:0]), dev(dest[:0]), dev(pjob[:0]), dev(pread[:0]), rec_t, dev(side), dev(calls), None, n)
    al.sync()


# ---- a realistic slice: the records of the recorded reference calls ------------------------------------------------------
def test_reference_call_records_through_the_reduce_and_middle_hits(al, goldens):
    """The records align_pairs returns for the recorded reference calls in tests/golden/, as end-window jobs of one batch
    and as whole-read records: trims, a barcode call and hits equal the reference's rules on their own strings."""
    S = goldens["strings"]
    calls = [c for c in goldens["calls"] if list(c[2]) == [3, -6, -5, -2]][:4096]
    ads = {}
    pairs = [(S[c[0]], ads.setdefault(c[1], len(ads))) for c in calls]
    import porechop_amd
    a2 = porechop_amd.Aligner([S[k] for k in ads])
    recs = a2.align_pairs(pairs)
    a2.close()
    F = glue_ref.record_fields(recs)
    for f, c in zip(F, calls):                               # the parsed fields are the reference's own string's
        parts = c[3].split(",")
        if int(parts[0]) != -1:
            assert repr(f) == repr((float(parts[6]), float(parts[5]), int(parts[0]), int(parts[1]) + 1))   # (nan == nan)
    n = len(recs) // 4
    J = 4
    offs, sides = [j * n for j in range(J)], [0, 1, 0, 1]
    bins = [(0, 1), (2, -1), (-1, 3)]
    FF = glue_ref.record_fields(recs[:J * n], score_only_fails=True)
    for thr, et_thr, two in ((75.0, 75.0, False), (0.0, 33.333333, True), (66.666667, 0.0, False)):
        p = (150, 10, 2, et_thr)
        got = run_reduce(al, recs[:J * n], offs, sides, bins, n, p, thr, 0.0, two)
        fields = [[FF[offs[j] + r] for j in range(J)] for r in range(n)]
        want = ([glue_ref.end_trims(fields[r], sides, *p)[0] for r in range(n)],
                [glue_ref.end_trims(fields[r], sides, *p)[1] for r in range(n)],
                [glue_ref.barcode_call(fields[r], bins, thr, 0.0, two) for r in range(n)])
        assert got == want
    for thr in (90.0, 75.0, 50.0):
        full, hit = al.middle_hits(dev(recs), thr)
        al.sync()
        assert hit.cpu().tolist() == [glue_ref.middle_hit(f, thr)[1] for f in F]
