"""Pipeline.phase_c on the GPU by both glues of porechop_amd/middle.py: the Aligner's kernels, as the process stands, and the
torch glue over the same device tensors (PC_NO_FUSED_GLUE=1, read per call).  One loop, one contract: hits, rounds,
alignment counts and the pair statistics are equal, on the default route and behind the exact prefilter.  The reads are those
of tests/test_mask_rule_pipeline_cpu.py (several rounds, overlapping hits of different sets, records that meet a mask by one
column), whose CPU run holds the torch glue to the reference's sequential logic."""
import pytest

from tests import maskgen

pytestmark = pytest.mark.gpu

CASES = [("junctions", maskgen.SETS, 75.0), ("junctions", maskgen.SETS, 85.0), ("touching", maskgen.SETS3, 90.0)]
STATS = ("pairs_middle", "pairs_middle_speculative")


@pytest.fixture(scope="module")
def inputs():
    return {"junctions": maskgen.reads(75, 36), "touching": maskgen.touching_reads(9, 16)}


def run(pl, dreads, matching, prefilter):
    import torch
    zero = torch.zeros(dreads.n, dtype=torch.int32, device="cuda")
    before = [pl.stats.get(k, 0) for k in STATS]
    h = pl.phase_c(dreads, zero, zero, matching, prefilter=prefilter)
    pl.aligner.sync()
    return h, [pl.stats.get(k, 0) - b for k, b in zip(STATS, before)]


@pytest.mark.parametrize("prefilter", [False, True])
@pytest.mark.parametrize("which,names,threshold", CASES)
def test_phase_c_is_the_same_by_the_native_glue_and_by_the_torch_glue(inputs, monkeypatch, which, names, threshold, prefilter):
    import torch
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import Pipeline, ScanParams
    from porechop_amd.synth import reads_from_strings
    pl = Pipeline(load_panel(), ScanParams(middle_threshold=threshold))
    try:
        matching = [i for i, s in enumerate(pl.sets) if s.name in names]
        assert len(matching) == len(names)
        dreads, _ = reads_from_strings(inputs[which])
        h0, stats0 = run(pl, dreads, matching, prefilter)
        monkeypatch.setenv("PC_NO_FUSED_GLUE", "1")
        h1, stats1 = run(pl, dreads, matching, prefilter)
    finally:
        pl.close()
    for f in ("read", "adapter", "start", "end", "identity"):
        assert torch.equal(getattr(h0, f), getattr(h1, f)), f
    assert (h0.rounds, h0.alignments) == (h1.rounds, h1.alignments)
    assert stats0 == stats1, (STATS, stats0, stats1)
    assert h0.read.numel() >= len(inputs[which]) // 2
    if which == "junctions":
        assert h0.rounds >= 3
