"""run(..., report=PATH) on the CPU: the reasons behind every trim and call against the reference's own per-read
attributes (tests/golden/explain_goldens.json.gz), with the alignments from the oracle through the Aligner-shaped
stand-in of tests/cpu_aligner.py (so the per-read pass is Pipeline's torch formulation; the HIP kernel is
tests/test_gpu_explain.py).  Plus the report itself: streamed = whole, the command line, no report in a sharded run."""
import pytest

from tests.cpu_aligner import OracleAligner
from tests.explain_cases import check_against_golden, coverage, load_goldens, run_with_report
from tests.runner_cases import GPU_ONLY, load_cases

# without barcodes + middle adapters / reads with two sets at an end / a barcode directory / --require_two_barcodes /
# an Albacore directory (the agreement rule of the final call)
CPU_CASES = ["ligation_default", "native_default", "native_bins", "native_bins_two", "albacore_bins"]


def test_fixture_is_not_trivial():
    cases = load_goldens()
    assert set(CPU_CASES) <= set(cases) and not (set(CPU_CASES) & GPU_ONLY)
    cov = coverage({k: cases[k] for k in CPU_CASES})
    assert all(cov.values()), cov
    assert any(not c["demultiplexed"] for c in cases.values())
    assert any("--require_two_barcodes" in c["argv"] for c in cases.values())


@pytest.mark.parametrize("name", CPU_CASES)
def test_report_matches_the_reference_read_by_read(oracle, tmp_path, name):
    golden = load_goldens()[name]
    case = load_cases()[name]
    assert (case["dataset"], case["argv"], case["input_sha1"]) == (golden["dataset"], golden["argv"], golden["input_sha1"])
    res, text, md5s = run_with_report(name, case, str(tmp_path), {}, make_aligner=lambda sc: OracleAligner(oracle, sc))
    assert md5s == case["outputs"], name                      # the output files are the ones of a run without a report
    check_against_golden(name, golden, res, text)


def test_streamed_report_equals_whole_run_report(oracle, tmp_path):
    """Small forced blocks: the report is appended block after block and comes out the same bytes; so do the arrays."""
    import numpy as np
    cases = load_cases()
    mk = lambda sc: OracleAligner(oracle, sc)
    bins20 = dict(cases["native_bins"], argv=["--check_reads", "20", "--adapter_threshold", "95"])
    for name, case in (("native_check20", cases["native_check20"]), ("native_bins_check20", bins20)):
        datasets = {}
        whole, text, md5s = run_with_report(name, case, str(tmp_path), datasets, make_aligner=mk)
        blocks = []
        from porechop_amd import runner
        real = runner.ReadSet.segment
        runner.ReadSet.segment = staticmethod(lambda p, b, t: (blocks.append(b), real(p, b, t))[1])
        try:
            part, text_s, md5s_s = run_with_report(name, case, str(tmp_path), datasets, make_aligner=mk, streamed_block=6000)
        finally:
            runner.ReadSet.segment = real
        assert len(blocks) > 10
        assert text_s == text and md5s_s == md5s, name
        assert text.count("\n") == whole.n_reads + 1
        for f in ("summary", "bscore", "hit_first", "hits", "middle_first", "middle", "middle_identity"):
            assert np.array_equal(getattr(part.explain, f), getattr(whole.explain, f)), (name, f)
        assert part.explain.calls == whole.explain.calls


def test_explain_command_line_writes_the_same_report(oracle, tmp_path, monkeypatch):
    """`python -m porechop_amd.explain`: the reference's options plus --report, over the same run()."""
    import porechop_amd.__main__ as cli
    from porechop_amd import explain, runner
    case = load_cases()["native_bins_two"]
    datasets = {}
    _, text, md5s = run_with_report("cli", case, str(tmp_path), datasets, make_aligner=lambda sc: OracleAligner(oracle, sc))
    seen = {}

    def run_with_stand_in(*a, **kw):
        seen.update(kw)
        return runner.run(*a, aligner=OracleAligner(oracle, kw["options"].scoring_scheme), **kw)
    monkeypatch.setattr(cli, "run", run_with_stand_in)
    report = str(tmp_path / "cli_report.tsv")
    explain.main(["-i", datasets[case["dataset"]], "-b", str(tmp_path / "cli_bins"), "-v", "0", "--report", report] + case["argv"])
    assert seen["report"] == report and seen["options"].require_two_barcodes
    assert open(report).read() == text
    with pytest.raises(SystemExit):                            # --report is required there ...
        explain.main(["-i", "x"])
    with pytest.raises(SystemExit):                            # ... and unknown to the reference's command line
        cli.main(["-i", "x", "--report", report])


def test_report_in_a_sharded_run_is_refused(tmp_path, monkeypatch):
    import torch.distributed as dist
    from porechop_amd import runner
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(runner.UsageError, match="sharded"):
        runner.run(str(tmp_path / "reads.fastq"), output=str(tmp_path / "out.fastq"), report=str(tmp_path / "r.tsv"))
    assert not (tmp_path / "r.tsv").exists()
