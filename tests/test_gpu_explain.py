"""pc_phase_b_explain on the MI355X: both passes element by element against the plain host model (tests/explain_ref.py)
on generated record tables and on the records of a real barcoded batch, consistent with pc_phase_b_reduce on the same
records, and the explain golden cases (the reference's own per-read attributes) through the HIP library."""
import numpy as np
import pytest

from tests import explain_ref, explaingen, gluegen
from tests.explain_cases import check_against_golden, load_goldens, run_with_report
from tests.runner_cases import load_cases

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ["ligation_default", "native_default", "native_bins", "native_bins_two", "albacore_bins", "native_loose"]


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    a = porechop_amd.Aligner(["ACGTACGTAC"])
    yield a
    assert a.lib.pc_sync(a._ctx, None) == 0                  # PC_OK: no kernel of this module reported anything
    a.close()


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_explain(al, recs, offs, sides, bins, n, p, mask=None):
    out = al.phase_b_explain(dev(recs), n, offs, sides, *p, bins=bins or None, traced_mask=None if mask is None else dev(mask))
    al.sync()
    return tuple(t.cpu().numpy() for t in out)


def compare(got, want, what):
    for name, g, w in zip(("summary", "bscore", "hit_first", "hits"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0] if g.size else []
        assert len(bad) == 0, (what, name, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


# (n, jobs, bins, one job serving several bins): n across the wave, the block and the 64-read mask word; no bins; the
# shape of a barcode panel
SHAPES = [(1, 1, 0, False), (63, 3, 1, False), (64, 7, 3, False), (65, 7, 2, True), (255, 24, 12, False), (257, 24, 5, True),
          (4097, 9, 4, False), (1000, 196, 96, False)]
PARAMS = [(150, 50, 2, 75.0), (150, 51, 0, 33.333333), (150, 1, 7, 0.0), (150, 50, 3, 100.0 / 3)]


@pytest.mark.parametrize("masked", [False, True])
def test_both_passes_equal_the_host_model(al, masked):
    seen_ties = seen_lists = 0
    for k, (n, J, nbins, shared) in enumerate(SHAPES):
        rng = np.random.default_rng(1000 + 2 * k + masked)
        recs, offs, sides, bins = explaingen.case(rng, n, J, nbins, shared_jobs=shared)
        mask = gluegen.traced_mask(rng, J, n) if masked else None
        bits = gluegen.unpack_bits(mask, n) if masked else None
        for p in (PARAMS if J < 100 else PARAMS[:1]):
            want = explain_ref.explain(recs, n, offs, sides, *p, bins=bins, traced=bits)
            compare(run_explain(al, recs, offs, sides, bins, n, p, mask), want, (n, J, nbins, shared, p, masked))
            s, b = want[0], want[1]
            seen_lists += int(((s[:, 2] >= 2) | (s[:, 3] >= 2)).sum())
            seen_ties += int(((s[:, 6] >= 0) & (s[:, 7] >= 0) & (b[:, 0] == b[:, 1])).sum())
    assert seen_lists > 100 and seen_ties > 20                # the constructed ties were really there


def test_zero_jobs_no_bins_and_an_empty_batch(al):
    import torch
    recs = np.zeros((4, 8), dtype=np.int32)
    summary, bscore, first, hits = run_explain(al, recs, [], [], [], 130, PARAMS[0])
    assert summary.shape == (130, 12) and (summary[:, 0:4] == 0).all() and (summary[:, 4:10] == -1).all() and (summary[:, 10:] == 0).all()
    assert (bscore == 0.0).all() and (first == 0).all() and hits.shape == (0, 6)
    # bins that all lack their entries: 'none' on both sides
    rng = np.random.default_rng(3)
    recs, offs, sides, _ = explaingen.case(rng, 70, 3, 0)
    got = run_explain(al, recs, offs, sides, [(-1, -1), (-1, -1)], 70, PARAMS[0])
    compare(got, explain_ref.explain(recs, 70, offs, sides, *PARAMS[0], bins=[(-1, -1), (-1, -1)]), "absent bins")
    assert (got[0][:, 6:10] == -1).all()
    out = al.phase_b_explain(torch.zeros((4, 8), dtype=torch.int32, device="cuda"), 0, [0], [0], *PARAMS[0])
    al.sync()
    assert [tuple(t.shape) for t in out] == [(0, 12), (0, 4), (1,), (0, 6)]


@pytest.mark.parametrize("masked", [False, True])
def test_consistent_with_phase_b_reduce(al, masked):
    """Fields 0 and 1 are pc_phase_b_reduce's trims, and the call that follows from the best / second-best bins and their
    scores is pc_phase_b_reduce's call, on the same records."""
    import torch
    for k, (n, J, nbins, shared) in enumerate([(257, 24, 12, False), (1000, 40, 9, True), (4097, 9, 4, False)]):
        rng = np.random.default_rng(50 + 2 * k + masked)
        recs, offs, sides, bins = explaingen.case(rng, n, J, nbins, shared_jobs=shared)
        mask = gluegen.traced_mask(rng, J, n) if masked else None
        d_recs, d_mask = dev(recs), (dev(mask) if masked else None)
        for p in PARAMS[:2]:
            summary, bscore, _, _ = run_explain(al, recs, offs, sides, bins, n, p, mask)
            for thr, diff, two in ((75.0, 5.0, False), (75.0, 5.0, True), (33.333333, 0.0, False), (0.0, 0.0, True), (66.666667, 100.0 / 3 - 33.333333, False)):
                st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                et = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                call = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                al.phase_b_reduce(d_recs, n, offs, sides, *p, st, et, bins=bins, barcode_threshold=thr, barcode_diff=diff, require_two=two,
                                  call=call, traced_mask=d_mask)
                al.sync()
                assert np.array_equal(st.cpu().numpy(), summary[:, 0]) and np.array_equal(et.cpu().numpy(), summary[:, 1])
                implied = [explain_ref.implied_call(summary[r], bscore[r], thr, diff, two) for r in range(n)]
                assert implied == call.cpu().tolist(), (n, J, p, thr, diff, two)


def test_records_of_a_real_barcoded_batch():
    """A barcoded batch through the library's own scans: every pair traced, and the pruned records with their traced mask."""
    import torch
    from porechop_amd import panel as rules
    from porechop_amd.batch import MODE_TRACE
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import Pipeline, ScanParams
    from porechop_amd.runner import barcode_bins
    from porechop_amd.synth import make_reads
    panel = load_panel()
    fw = [s for s in panel if s.name.startswith("Barcode ") and "(forward)" in s.name]
    pl = Pipeline(panel, ScanParams())
    try:
        p = pl.p
        reads = make_reads(1500, 3000, seed=21, start_frac=0.9, end_frac=0.5, chimera_frac=0.0,
                           barcodes_start=[s.start[1] for s in fw], barcodes_end=[s.end[1] for s in fw])
        R = reads.n
        matching = [i for i, s in enumerate(pl.sets) if s.name == "SQK-NSK007" or s in fw]
        names, bins = barcode_bins(pl, [i for i in matching if rules.is_barcode(pl.sets[i])])
        jobs, where = pl._phase_b_jobs(reads, matching)
        sides = [w[0] for w in where]
        job_of = {(si, side): k for k, (side, si) in enumerate(where)}
        jb = [(job_of.get((b[0], 0), -1), job_of.get((b[1], 1), -1)) for b in bins]
        args = (p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold)
        # every pair traced: the route of the report
        _, rec, rec_off = pl._scan_jobs(pl._ends_arena(reads), jobs, MODE_TRACE, p.end_size, with_layout=True)
        got = pl.aligner.phase_b_explain(rec, R, rec_off, sides, *args, bins=jb)
        pl.aligner.sync()
        want = explain_ref.explain(rec.cpu().numpy(), R, rec_off, sides, *args, bins=jb)
        compare(tuple(t.cpu().numpy() for t in got), want, "traced")
        assert int(want[2][-1]) > R and (want[0][:, 7] >= 0).all()
        st_e, et_e, call_e, ex = pl.phase_b_explain(reads, matching, bins, 75.0, 5.0, False)
        assert np.array_equal(ex.summary.cpu().numpy(), want[0]) and np.array_equal(ex.hits.cpu().numpy(), want[3])
        # the pruned records: the same trims and the same best barcode; the lists hold what was traced
        st_p, et_p, call_p = pl.phase_b_demux(reads, matching, bins, 75.0, 5.0, False, prune=True)
        assert torch.equal(st_p, st_e) and torch.equal(et_p, et_e) and np.array_equal(call_p, call_e)

        def trims(records, offs, mask=None):
            a = torch.zeros(R, dtype=torch.int32, device="cuda")
            b = torch.zeros(R, dtype=torch.int32, device="cuda")
            pl.aligner.phase_b_reduce(records, R, offs, sides, *args, a, b, traced_mask=mask.contiguous())
            return a, b
        call_sets = {i for b in bins for i in b if i is not None}
        prec, poff = pl._phase_b_pruned_records(reads, jobs, where, call_sets, 70.0, trims, call_level_diff=5.0)
        mask = pl._traced_mask.contiguous()
        got = pl.aligner.phase_b_explain(prec, R, poff, sides, *args, bins=jb, traced_mask=mask)
        pl.aligner.sync()
        bits = gluegen.unpack_bits(mask.cpu().numpy(), R)
        assert bits.mean() < 0.5
        wantp = explain_ref.explain(prec.cpu().numpy(), R, poff, sides, *args, bins=jb, traced=bits)
        compare(tuple(t.cpu().numpy() for t in got), wantp, "pruned")
        assert np.array_equal(wantp[0][:, 0:2], want[0][:, 0:2])
        assert pl.aligner.lib.pc_sync(pl.aligner._ctx, None) == 0
    finally:
        pl.close()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_cases_on_the_device(tmp_path, name):
    golden = load_goldens()[name]
    case = load_cases()[name]
    res, text, md5s = run_with_report(name, case, str(tmp_path), {}, device="cuda")
    assert md5s == case["outputs"], name
    check_against_golden(name, golden, res, text)


def test_streamed_report_and_command_line_on_the_device(tmp_path):
    import os
    import subprocess
    import sys
    cases = load_cases()
    case = cases["native_check20"]
    datasets = {}
    whole, text, md5s = run_with_report("check20", case, str(tmp_path), datasets, device="cuda")
    part, text_s, md5s_s = run_with_report("check20", case, str(tmp_path), datasets, device="cuda", streamed_block=6000)
    assert text_s == text and md5s_s == md5s == case["outputs"]
    case = cases["native_bins_two"]
    _, text, _ = run_with_report("two", case, str(tmp_path), datasets, device="cuda")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    report = str(tmp_path / "cli.tsv")
    res = subprocess.run([sys.executable, "-m", "porechop_amd.explain", "-i", datasets[case["dataset"]], "-b", str(tmp_path / "cli_bins"),
                          "--report", report] + case["argv"], cwd=repo, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert open(report).read() == text
