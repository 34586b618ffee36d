"""The mask rounds of Pipeline.phase_c with the mask rule (csrc/pc_mask_rule.h), on the oracle stand-in: a round scans, per
adapter set, only the reads that have a record of the set the mask can have changed.  Hits, rounds and alignment counts are
those of the rounds that realign everything (PC_NO_MASK_RULE=1) and of the reference's sequential logic; fewer pairs are
launched; an adapter list the rule's gate refuses (a letter N) launches what it launched before.  Host logic only: the torch
formulation of the selection, which an aligner without the native step takes; the same on the GPU in tests/test_gpu_mask_rule.py."""
import numpy as np
import pytest
import torch

from tests import maskgen, ref_pipeline
from tests.cpu_aligner import OracleAligner


class CountingAligner(OracleAligner):
    """Counts the (window, adapter) pairs every scan call is asked for."""
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def scan_device(self, arena, win_off, win_len, job_adapter, job_start, max_len, out, mode=0, stream=None, job_adapter_b=None):
        n = 0
        for k in range(len(job_adapter)):
            w = int(job_start[k + 1]) - int(job_start[k])
            n += w * (2 if job_adapter_b is not None and int(job_adapter_b[k]) >= 0 else 1)
        self.calls.append(n)
        return super().scan_device(arena, win_off, win_len, job_adapter, job_start, max_len, out, mode, stream, job_adapter_b)


def device_reads(seqs):
    from porechop_amd.pipeline import DeviceReads
    arena = np.frombuffer(("".join(seqs)).encode() + b"N" * 64, dtype=np.uint8).copy()
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
    return DeviceReads(torch.from_numpy(arena), torch.from_numpy(offs), torch.from_numpy(lens))


def run(oracle, monkeypatch, sets, names, seqs, threshold, rule):
    from porechop_amd.pipeline import Pipeline, ScanParams
    if rule:
        monkeypatch.delenv("PC_NO_MASK_RULE", raising=False)
    else:
        monkeypatch.setenv("PC_NO_MASK_RULE", "1")
    p = ScanParams(middle_threshold=threshold)
    al = CountingAligner(oracle, p.scores)
    pl = Pipeline(sets, p, aligner=al)
    matching = [i for i, s in enumerate(pl.sets) if s.name in names]
    assert len(matching) == len(names)
    zero = torch.zeros(len(seqs), dtype=torch.int32)
    h = pl.phase_c(device_reads(seqs), zero, zero, matching)
    return pl, h, al.calls


def same_hits(h0, h1):
    for f in ("read", "adapter", "start", "end", "identity"):
        assert torch.equal(getattr(h0, f), getattr(h1, f)), f
    assert (h0.rounds, h0.alignments) == (h1.rounds, h1.alignments)


@pytest.mark.parametrize("threshold", [75.0, 85.0])
def test_rounds_with_the_rule_equal_the_rounds_without_and_the_reference(oracle, monkeypatch, threshold):
    from porechop_amd.panel import load_panel
    seqs = maskgen.reads(int(threshold), 36)
    pl1, h1, calls1 = run(oracle, monkeypatch, load_panel(), maskgen.SETS, seqs, threshold, rule=True)
    pl0, h0, calls0 = run(oracle, monkeypatch, load_panel(), maskgen.SETS, seqs, threshold, rule=False)
    same_hits(h0, h1)
    assert h1.rounds >= 3 and h1.read.numel() >= 30
    # round 0 is the same call; the mask rounds launch fewer pairs, and the new statistic says how many fewer
    assert calls1[0] == calls0[0] and len(calls1) >= 3
    assert sum(calls1) < sum(calls0)
    assert pl1.stats["pairs_middle_kept_by_mask_rule"] == sum(calls0) - sum(calls1) > 0
    assert pl0.stats["pairs_middle_kept_by_mask_rule"] == 0
    assert pl1.stats["pairs_middle_speculative"] == pl0.stats["pairs_middle_speculative"]      # (today's definition: not what was launched)
    assert pl1.stats["pairs_middle"] == pl0.stats["pairs_middle"]
    # the reference's nested loops, read by read; two adapters of different sets do hit overlapping intervals here
    got = {}
    for r, a, s, e, idn in zip(h1.read.tolist(), h1.adapter.tolist(), h1.start.tolist(), h1.end.tolist(), h1.identity.tolist()):
        got.setdefault(r, []).append((a, s, e, round(idn, 6)))
    first_base = last_base = 0
    for r, seq in enumerate(seqs):
        want = [(a, s, e, round(f, 6)) for a, s, e, f in ref_pipeline.phase_c(oracle.adapter_alignment, seq, 0, 0, pl1.middle_adapters, pl1.p)]
        assert got.get(r, []) == want, (r, got.get(r), want)
        first_base += any(s == 0 for _, s, _, _ in want)
        last_base += any(e == len(seq) for _, _, e, _ in want)
    assert first_base >= 2 and last_base >= 2
    # ... asserted on the unmasked reads' own records: reads in which two adapters of DIFFERENT sets both reach the threshold
    # over intervals that share columns, so that the mask of the first hit takes the second one's record
    ads = pl1.middle_adapters
    set_of = {0: 0, 1: 0, 2: 1, 3: 1}
    assert [a[1] for a in ads] == [maskgen.Y_TOP, maskgen.Y_BOTTOM, maskgen.P2_START, maskgen.P2_END]
    overlapping = 0
    for seq in seqs:
        recs = [ref_pipeline.align_adapter(oracle.adapter_alignment, seq, a[1], pl1.p.scores) for a in ads]
        hit = [(k, rs, re) for k, (full, _, rs, re) in enumerate(recs) if rs != -1 and full >= threshold]
        overlapping += any(set_of[k] != set_of[j] and rs < re2 and rs2 < re for k, rs, re in hit for j, rs2, re2 in hit)
    assert overlapping >= 3, overlapping


def test_an_adapter_with_n_keeps_the_rounds_as_they_were(oracle, monkeypatch):
    """N equals N and a masked base codes as N: masking can RAISE such an adapter's score (tests/host/test_mask_rule.cpp), so the
    gate refuses the whole list and every round realigns everything."""
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import AdapterSet
    sets = load_panel() + [AdapterSet("custom with N", ("custom_n", "AATGTACTNNNNCAGTTACGTATTGCT"), None)]
    names = maskgen.SETS + ("custom with N",)
    seqs = maskgen.reads(5, 16)
    pl1, h1, calls1 = run(oracle, monkeypatch, sets, names, seqs, 85.0, rule=True)
    pl0, h0, calls0 = run(oracle, monkeypatch, sets, names, seqs, 85.0, rule=False)
    same_hits(h0, h1)
    assert h1.rounds >= 2 and calls1 == calls0
    assert pl1.stats["pairs_middle_kept_by_mask_rule"] == 0


def test_records_that_meet_the_mask_by_one_column_are_realigned(oracle, monkeypatch):
    """A barcode copy that shares its first (last) base with the last (first) base of the 28-mer's hit: the mask takes one
    column of the barcode's record, which changes (23 of 24 bases are left).  Kept, the stale record would be the next hit."""
    from porechop_amd.panel import load_panel
    seqs = maskgen.touching_reads(9, 16)
    pl1, h1, calls1 = run(oracle, monkeypatch, load_panel(), maskgen.SETS3, seqs, 90.0, rule=True)
    pl0, h0, calls0 = run(oracle, monkeypatch, load_panel(), maskgen.SETS3, seqs, 90.0, rule=False)
    same_hits(h0, h1)
    assert sum(calls1) < sum(calls0)
    got = {}
    for r, a, s, e, idn in zip(h1.read.tolist(), h1.adapter.tolist(), h1.start.tolist(), h1.end.tolist(), h1.identity.tolist()):
        got.setdefault(r, []).append((a, s, e, round(idn, 6)))
    changed = 0
    for r, seq in enumerate(seqs):
        want = [(a, s, e, round(f, 6)) for a, s, e, f in ref_pipeline.phase_c(oracle.adapter_alignment, seq, 0, 0, pl1.middle_adapters, pl1.p)]
        assert got.get(r, []) == want, (r, got.get(r), want)
        assert len(want) == 2 and want[0][0] == 0 and want[1][0] in (4, 5), want
        changed += want[1][3] < 100.0                            # the barcode's hit lost the shared base to the mask
    assert changed >= 10


def test_the_torch_rule_is_the_headers_rule():
    """The selection an aligner without the native step takes (pipeline.must_realign_torch) against pcm::must_realign as the
    library compiles it, record by record: random records and the edges -- "no alignment" floored and unfloored, empty
    masks, odd records, intervals that meet the mask by 0 and 1 columns on either side, adapters below, at and above the hit."""
    import random
    from porechop_amd.batch import mask_rule_must_realign
    from porechop_amd.pipeline import must_realign_torch
    rng = random.Random(17)
    rows = []
    for _ in range(4000):
        rs = rng.randrange(0, 300)
        re = rs + rng.choice((0, 0, 1, 2, 22, 28, 40))
        kind = rng.randrange(8)
        if kind == 0:
            r0, r1 = -1, 0
        elif kind == 1:
            r1 = rs - rng.choice((0, 1)); r0 = r1 - rng.randrange(0, 30)
        elif kind == 2:
            r0 = re - rng.choice((0, 1)); r1 = r0 + rng.randrange(0, 30)
        elif kind == 3:
            r0 = rng.randrange(0, 300); r1 = r0 - rng.randrange(1, 4)
        else:
            r0 = rng.randrange(-3, 340); r1 = r0 + rng.randrange(0, 40)
        rows.append((rng.randrange(0, 6), rng.randrange(0, 6), r0, r1, rs, re))
    a, cur, r0, r1, rs, re = (torch.tensor(col) for col in zip(*rows))
    for floored in (False, True):
        got = must_realign_torch(a, cur, r0, r1, rs, re, floored).tolist()
        want = [mask_rule_must_realign(*row, floored) for row in rows]
        bad = [(row, g, w) for row, g, w in zip(rows, got, want) if g != w]
        assert not bad, (floored, bad[:5])
        assert 0 < sum(want) < len(want)


def test_a_barcode_panel_of_many_sets(oracle, monkeypatch):
    """Many adapter sets, as a barcoded run has them: one window list per set that needs a scan, dozens of jobs with different
    lists in one call, records scattered back job by job.  The hits are those of the rounds that realign everything and of the
    reference's sequential logic."""
    import random
    from porechop_amd.panel import load_panel
    panel = load_panel()
    barcodes = tuple(s.name for s in panel if s.name.startswith("Barcode ") and "(reverse)" in s.name)[:12]
    names = maskgen.SETS + barcodes
    by_name = {s.name: s for s in panel}
    rng = random.Random(23)
    seqs = []
    for i in range(24):
        parts = [maskgen._bases(rng, rng.randrange(60, 200))]
        for _ in range(rng.randrange(1, 5)):
            s = by_name[rng.choice(names)]
            parts += [maskgen._mutate(rng, rng.choice((s.start, s.end))[1], rng.choice((0.0, 0.0, 0.05))), maskgen._bases(rng, rng.randrange(0, 120))]
        seqs.append("".join(parts))
    pl1, h1, calls1 = run(oracle, monkeypatch, panel, names, seqs, 85.0, rule=True)
    pl0, h0, calls0 = run(oracle, monkeypatch, panel, names, seqs, 85.0, rule=False)
    same_hits(h0, h1)
    assert len(pl1.middle_adapters) == 28 and h1.rounds >= 3 and h1.read.numel() >= 40
    assert sum(calls1[1:]) * 4 < sum(calls0[1:])                 # most of the 28 adapters' records are kept
    got = {}
    for r, a, s, e, idn in zip(h1.read.tolist(), h1.adapter.tolist(), h1.start.tolist(), h1.end.tolist(), h1.identity.tolist()):
        got.setdefault(r, []).append((a, s, e, round(idn, 6)))
    for r, seq in enumerate(seqs):
        want = [(a, s, e, round(f, 6)) for a, s, e, f in ref_pipeline.phase_c(oracle.adapter_alignment, seq, 0, 0, pl1.middle_adapters, pl1.p)]
        assert got.get(r, []) == want, (r, got.get(r), want)
