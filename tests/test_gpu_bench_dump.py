"""The plain `bench.py` run: only the headline region, exactly --steps timed steps, and with --dump-outputs DIR the arrays
the last timed step returned -- the same ones, bit for bit, from two runs with the same arguments (the reads are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("matching_sets", "start_trim", "end_trim", "middle_hit_read", "middle_hit_adapter", "middle_hit_start",
         "middle_hit_end", "middle_hit_identity", "middle_hit_rounds_alignments")


def _plain(out_dir, reads=100000):
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--reads", str(reads), "--dump-outputs", str(out_dir)]
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    a = _plain(tmp_path / "a")
    b = _plain(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "reads/s" and d["higher_is_better"] is True and d["metric"] and d["dtype"]
        assert d["legs"] == {} and "cpu_baseline" not in d                  # nothing beside the headline without --full
    assert a["config"]["middle_hits_per_step"] == b["config"]["middle_hits_per_step"] > 0
    total = 0
    for name in NAMES:
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float64 and np.array_equal(x, y), name
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64 << 20
    st, et = np.load(tmp_path / "a" / "start_trim.npy"), np.load(tmp_path / "a" / "end_trim.npy")
    assert st.shape == et.shape == (100000,) and st.max() > 0
    assert np.load(tmp_path / "a" / "middle_hit_read.npy").size == a["config"]["middle_hits_per_step"]
    assert np.load(tmp_path / "a" / "matching_sets.npy").size >= 1
