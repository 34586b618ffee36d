"""The row skip of the floored middle scan's score pass (csrc/pc_bounds.h row_skip_plan, the row-skipping variant of
pc_spec_score): records of pairs at or above their floor, the floor counter and everything phase C reports are what they are
without it.

Scan level (tests/row_skip_child.py, one child process that pins the specialised packed-fp16 kernels): floored two-pass
calls with the skip against the same call under PC_NO_ROW_SKIP=1, against the unfloored call and against the oracle, over
batches that plant the edges, with the debug counters' on-fraction.  Pipeline level: phase_c with the skip, without it and
the reference's sequential logic on the oracle give the same middle hits."""
import os
import random
import subprocess
import sys

import pytest

from tests import floorgen, ref_pipeline
from tests.golden_io import load_panel
from tests.test_gpu_pass2_floor import chimeric_reads

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_skipping_scan_equals_the_plain_floored_scan_in_a_child_process(tmp_path):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    for k in ("PC_DISABLE_JIT", "PC_FORCE_CHUNKS", "PC_NO_PASS2_FLOOR", "PC_DISABLE_F16", "PC_NO_ROW_SKIP", "PC_JIT_INT16", "PC_JIT_R0",
              "PC_JIT_CHECK_RANGE"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "tests.row_skip_child"], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert res.returncode == 0 and "ROW_SKIP_CHILD_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def test_phase_c_same_hits_with_and_without_the_row_skip(oracle, monkeypatch):
    import torch
    from porechop_amd.pipeline import AdapterSet, Pipeline, ScanParams
    from porechop_amd.synth import reads_from_strings

    for k in ("PC_NO_PASS2_FLOOR", "PC_NO_ROW_SKIP"):
        monkeypatch.delenv(k, raising=False)
    sets = [AdapterSet(a["name"], tuple(a["start"]) if a["start"] else None, tuple(a["end"]) if a["end"] else None) for a in load_panel()]
    p = ScanParams()
    pl = Pipeline(sets, p)
    matching = [i for i, s in enumerate(pl.sets) if s.name in floorgen.SETS]
    raw = chimeric_reads(random.Random(131), 131)
    dreads, norm = reads_from_strings(raw)
    zero = torch.zeros(len(raw), dtype=torch.int32, device="cuda")

    def run():
        h = pl.phase_c(dreads, zero, zero, matching)
        pl.aligner.sync()
        return h

    pl.aligner.set_row_skip_debug(True)
    h1 = run()
    skipped = pl.stats.get("pairs_middle_skipped_by_floor", 0)
    assert skipped > 0
    assert pl.aligner.row_skip_blocks()[0] > 0                      # the row-skipping kernels ran (not the generic one)
    monkeypatch.setenv("PC_NO_ROW_SKIP", "1")
    h0 = run()
    assert pl.aligner.row_skip_blocks() == (0, 0)
    assert pl.stats.get("pairs_middle_skipped_by_floor", 0) == 2 * skipped      # the same pairs below their floors
    assert h0.read.numel() >= 15
    for f in ("read", "adapter", "start", "end", "identity"):
        assert torch.equal(getattr(h0, f), getattr(h1, f)), f
    assert (h0.rounds, h0.alignments) == (h1.rounds, h1.alignments)
    got = {}
    for r, a, s, e, idn in zip(h1.read.cpu().tolist(), h1.adapter.cpu().tolist(), h1.start.cpu().tolist(), h1.end.cpu().tolist(),
                               h1.identity.cpu().tolist()):
        got.setdefault(r, []).append((a, s, e, round(idn, 6)))
    for r, seq in enumerate(norm):
        want = [(a, s, e, round(f, 6)) for a, s, e, f in ref_pipeline.phase_c(oracle.adapter_alignment, seq, 0, 0, pl.middle_adapters, p)]
        assert got.get(r, []) == want, (r, got.get(r), want)
    pl.close()
