"""The score floor of the middle scan's second pass (pc_scan_device_floored): pairs whose best score cannot mean a hit are
not traced, and nothing else changes.

Scan level (tests/floor_child.py, one child process that pins the generic and the specialised score kernel in turn): every
pair of a floored call against the unfloored call and the oracle's scores, fp16 and int16 lanes, uniform and ragged
lengths, the edge layouts.  Pipeline level: phase_c with the floor, without it (PC_NO_PASS2_FLOOR=1) and the reference's
sequential logic on the oracle give the same middle hits, rounds and alignment counts."""
import os
import random
import subprocess
import sys

import pytest

from tests import floorgen, ref_pipeline
from tests.golden_io import load_panel

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_floored_scan_equals_unfloored_scan_in_a_child_process(tmp_path):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    for k in ("PC_DISABLE_JIT", "PC_FORCE_CHUNKS", "PC_NO_PASS2_FLOOR", "PC_DISABLE_F16"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "tests.floor_child"], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert res.returncode == 0 and "FLOOR_GENERIC_OK" in res.stdout and "FLOOR_SPEC_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def chimeric_reads(rng, n):
    """n reads of 300..2000 random bases; 8 % carry a junction of two adapters, some of those one or two more copies far from
    it (reads with two and three hits: mask rounds 2 and 3)."""
    ads = [a[1] for a in floorgen.middle_adapters()]
    reads = []
    for i in range(n):
        ln = rng.randint(300, 2000)
        body = floorgen.random_bases(rng, ln)
        if i % 12 == 0:
            extra = (i // 12) % 3                                # 0, 1 or 2 further copies
            ln = max(ln, 900)
            body = floorgen.random_bases(rng, ln)
            at = [ln // 2] + [ln // 6, 5 * ln // 6][:extra]
            for k, pos in enumerate(sorted(at, reverse=True)):
                a, b = ads[(i + k) % 4], ads[(i + k + 1) % 4]
                piece = floorgen.edit(rng, a, rng.randint(0, 1)) + (floorgen.edit(rng, b, rng.randint(0, 1)) if pos == ln // 2 else "")
                body = body[:pos] + piece + body[pos:]
        elif i % 5 == 0:                                         # near misses: copies whose identity falls short
            a = ads[i % 4]
            pos = rng.randint(50, ln - 50)
            body = body[:pos] + floorgen.edit(rng, a, rng.randint(4, 8)) + body[pos:]
        reads.append(body)
    return reads


def test_phase_c_same_hits_with_and_without_the_floor(oracle, monkeypatch):
    import torch
    from porechop_amd.pipeline import AdapterSet, Pipeline, ScanParams
    from porechop_amd.synth import reads_from_strings

    monkeypatch.delenv("PC_NO_PASS2_FLOOR", raising=False)
    sets = [AdapterSet(a["name"], tuple(a["start"]) if a["start"] else None, tuple(a["end"]) if a["end"] else None) for a in load_panel()]
    p = ScanParams()
    pl = Pipeline(sets, p)
    matching = [i for i, s in enumerate(pl.sets) if s.name in floorgen.SETS]
    assert len(matching) == 2
    raw = chimeric_reads(random.Random(257), 257)
    dreads, norm = reads_from_strings(raw)
    zero = torch.zeros(len(raw), dtype=torch.int32, device="cuda")

    def run():
        h = pl.phase_c(dreads, zero, zero, matching)
        pl.aligner.sync()
        return h

    h1 = run()
    skipped = pl.stats.get("pairs_middle_skipped_by_floor", 0)
    assert skipped > 0
    monkeypatch.setenv("PC_NO_PASS2_FLOOR", "1")
    h0 = run()
    assert pl.stats.get("pairs_middle_skipped_by_floor", 0) == skipped          # nothing skipped without the floor
    assert h0.read.numel() >= 30
    for f in ("read", "adapter", "start", "end", "identity"):
        assert torch.equal(getattr(h0, f), getattr(h1, f)), f
    assert (h0.rounds, h0.alignments) == (h1.rounds, h1.alignments)
    assert h1.rounds >= 3                                                       # a read with three hits

    got = {}
    for r, a, s, e, idn in zip(h1.read.cpu().tolist(), h1.adapter.cpu().tolist(), h1.start.cpu().tolist(), h1.end.cpu().tolist(),
                               h1.identity.cpu().tolist()):
        got.setdefault(r, []).append((a, s, e, round(idn, 6)))
    calls = [0]

    def counting(*a):
        calls[0] += 1
        return oracle.adapter_alignment(*a)

    per_read = []
    for r, seq in enumerate(norm):
        want = [(a, s, e, round(f, 6)) for a, s, e, f in ref_pipeline.phase_c(counting, seq, 0, 0, pl.middle_adapters, p)]
        assert got.get(r, []) == want, (r, got.get(r), want)
        per_read.append(len(want))
    assert h1.alignments == calls[0]
    assert 2 in per_read and max(per_read) >= 3
    pl.close()
