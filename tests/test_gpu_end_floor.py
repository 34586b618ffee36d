"""Phase B with its rule handed to the end-window scan (pc_scan_device_end_rule): pairs whose score record proves that they
cannot trim their read are not traced, and nothing else changes.

Every batch (tests/end_floor_child.py: check_batch) runs phase B with the rule (end_rule=True: the default takes it from
END_RULE_MIN_READS reads on), with PC_NO_END_FLOOR=1, by default and through the reference's sequential logic on the
oracle, and compares the two scans record by record: a skipped pair has no trim of its own in the unruled traced scan,
every other record is identical, and the library's count of skipped pairs is the pipeline's.  Read counts 1, 63, 64, 65, 129 and 1 000; read lengths 0, 3, 40, 149, 150, 151 and 400; the headline's two
sets, a set with one sequence and a 24-mer pair.  One batch holds pairs exactly on the identity bound (found with the
oracle); one child process runs the scan over the generic, the shipped and the run-time-compiled score kernels."""
import math
import os
import random
import subprocess
import sys

import pytest

from tests import end_floor_child as gen

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pipeline():
    from porechop_amd.pipeline import Pipeline, ScanParams
    assert "PC_NO_END_FLOOR" not in os.environ
    pl = Pipeline(gen.sets(), ScanParams())
    yield pl
    pl.close()


@pytest.mark.parametrize("count", gen.COUNTS)
def test_trims_equal_unruled_and_reference(pipeline, oracle, count):
    raw = gen.make_reads(100 + count, count, pipeline.sets)
    assert len(raw) == count and len(raw[0]) == 400
    if count >= 63:
        assert {len(r) for r in raw} == set(gen.LENS)
    pairs, skipped, want, _, _ = gen.check_batch(pipeline, raw, oracle)
    assert pairs == 7 * count                                   # 2 + 2 + 1 + 2 (sequence, side) jobs
    assert 0 < skipped < pairs, (skipped, pairs)
    if count >= 63:
        assert sum(1 for s, e in want if s > 0) >= count // 8 and sum(1 for s, e in want if e > 0) >= count // 16


def test_pairs_exactly_on_the_identity_bound(pipeline, oracle):
    """Start windows whose alignment with the 28-mer has S == need and S == need + 1, need = floor(c min(I, Jc)): the first
    cannot reach the identity threshold and is skipped, the second is traced."""
    p = pipeline.p
    match, mismatch, go, ge = p.scores
    tau = (p.end_threshold - 1e-6) / 100.0
    c = tau * match - (1.0 - tau) * max(-mismatch, -go, -ge, 0)
    assert c > 0
    ad = pipeline.sets[0].start[1]
    assert pipeline.sets[0].name == "SQK-NSK007" and len(ad) == 28
    rng = random.Random(5)
    at, above = [], []
    for _ in range(20000):
        if len(at) >= 3 and len(above) >= 3:
            break
        w = gen.bases(rng, 150)
        if rng.random() < 0.7:
            w = gen.paste(w, rng.randint(5, 100), gen.mutate(rng, ad, rng.choice([0.2, 0.3, 0.4, 0.5])))
        r = oracle.align_raw(w, ad, p.scores)
        # (the rule's other conditions hold: the path ends inside the window, at least min_trim_size columns in)
        if r.failed or not (p.min_trim_size <= r.end_j + 1 and r.end_j < 150):
            continue
        need = math.floor(c * max(1, min(r.end_i, r.end_j)))
        if r.score == need and len(at) < 3:
            at.append(w)
        elif r.score == need + 1 and len(above) < 3:
            above.append(w)
    assert len(at) == 3 and len(above) == 3
    raw = [w + gen.bases(rng, 250) for w in at + above] + gen.make_reads(77, 59, pipeline.sets)
    pairs, skipped, _, ruled, full = gen.check_batch(pipeline, raw, oracle)
    job = 0                                                     # the first job: the first set's start sequence
    for r in range(3):
        assert ruled[job, r].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and int(full[job, r, 0]) != -1, (r, ruled[job, r].tolist())
    for r in range(3, 6):
        assert int(ruled[job, r, 0]) != -1 and ruled[job, r].tolist() == full[job, r].tolist(), (r, ruled[job, r].tolist())


def test_each_kind_of_score_kernel_in_a_child_process(tmp_path):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    for k in ("PC_DISABLE_JIT", "PC_FORCE_CHUNKS", "PC_NO_END_FLOOR", "PC_DISABLE_F16", "PC_JIT_INT16"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "tests.end_floor_child"], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert res.returncode == 0 and all(k in res.stdout for k in ("END_FLOOR_GENERIC_OK", "END_FLOOR_CACHED_OK", "END_FLOOR_COMPILED_OK")), \
        res.stdout[-2000:] + res.stderr[-4000:]
