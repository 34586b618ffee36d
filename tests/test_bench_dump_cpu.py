"""bench.dump_outputs on host tensors (no GPU needed): float64 files, nothing rounded, and over the size cap a fixed, seeded
sample of the per-read and per-hit rows with the indices kept."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402
from porechop_amd.pipeline import MiddleHits  # noqa: E402


def _outputs(n_reads, n_hits):
    g = torch.Generator().manual_seed(7)
    st = torch.randint(0, 200, (n_reads,), dtype=torch.int32, generator=g)
    et = torch.randint(0, 200, (n_reads,), dtype=torch.int32, generator=g)
    hits = MiddleHits(torch.randint(0, n_reads, (n_hits,), dtype=torch.int64, generator=g),
                      torch.randint(0, 4, (n_hits,), dtype=torch.int32, generator=g),
                      torch.randint(0, 8000, (n_hits,), dtype=torch.int32, generator=g),
                      torch.randint(0, 8000, (n_hits,), dtype=torch.int32, generator=g),
                      torch.rand(n_hits, dtype=torch.float64, generator=g) * 100, 2, 12345)
    return [3, 17], st, et, hits


def test_small_outputs_are_written_whole(tmp_path):
    matching, st, et, hits = _outputs(1000, 30)
    bench.dump_outputs(str(tmp_path), matching, st, et, hits)
    assert np.load(tmp_path / "matching_sets.npy").tolist() == [3.0, 17.0]
    assert np.array_equal(np.load(tmp_path / "start_trim.npy"), st.numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "end_trim.npy"), et.numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "middle_hit_identity.npy"), hits.identity.numpy())
    assert np.load(tmp_path / "middle_hit_rounds_alignments.npy").tolist() == [2.0, 12345.0]
    assert all(np.load(tmp_path / f).dtype == np.float64 for f in os.listdir(tmp_path))
    assert not os.path.exists(tmp_path / "read_sample.npy")


def test_large_outputs_keep_a_seeded_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 << 20)
    matching, st, et, hits = _outputs(200000, 5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), matching, st, et, hits, prefix="rank0_")
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 2 << 20
    for f in files:
        assert f.startswith("rank0_") and np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    keep = np.load(tmp_path / "a" / "rank0_read_sample.npy").astype(np.int64)
    assert 0 < keep.size < 200000 and np.all(np.diff(keep) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rank0_start_trim.npy"), st.numpy()[keep].astype(np.float64))
    hk = np.load(tmp_path / "a" / "rank0_hit_sample.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "rank0_middle_hit_read.npy"), hits.read.numpy()[hk].astype(np.float64))
