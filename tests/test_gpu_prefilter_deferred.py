"""The deferred overflow verdict of the prefilter's seed stage (pc_prefilter_defer_count / pc_prefilter_overflowed) and
the pipeline's re-run when it says the mask is incomplete.  Each test runs in a child process of its own: the seed
list's capacity (PC_PF_SEED_CAP) is read once per process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_VERDICT = r"""
import random, sys
sys.path.insert(0, %r)
import numpy as np
import torch
import porechop_amd
from tests.test_gpu_packed import _packed_plane
from tests.test_gpu_prefilter import make_cases

rng = random.Random(5)
adapters = ["AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT", "".join(rng.choice("ACGT") for _ in range(24)),
            "".join(rng.choice("ACGT") for _ in range(32)), "AAAAAAAAAAAAAAAAAAAAAAAA"]
edits = [3, 2, 2, 3, 2]
dev = torch.device("cuda")
# poly-A reads against a low-complexity adapter: far more seed candidates than a 64-entry list holds
overflowing = [r.replace("-", "A") for r in make_cases(31, 1500, [0, 5, 17, 150, 151, 600, 2500], adapters)] + ["A" * 3000, "ACGT" * 500]
calm = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(3)]
al = porechop_amd.Aligner(adapters)


def masks(reads, ids, ks):
    arr = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    d_off, d_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    arena = torch.from_numpy(np.concatenate([arr, np.full(64, ord("N"), np.uint8)])).to(dev)
    plane = _packed_plane(arr, dev)[0]
    mx = int(lens.max())
    out = {}
    for route in ("bytes", "packed"):
        def call(defer):
            al.prefilter_defer_count(defer)
            try:
                if route == "bytes":
                    m = al.prefilter_mask(arena, d_off, d_len, mx, ids, ks)
                else:
                    m = al.prefilter_mask_packed(plane, d_off, d_len, mx, ids, ks)
                    assert m is not None
            finally:
                al.prefilter_defer_count(False)
            al.sync()
            return m.cpu().numpy(), al.prefilter_overflowed()
        deferred, verdict = call(True)
        plain, after = call(False)
        out[route] = (deferred, verdict, plain, after)
    return out

ids = list(range(len(adapters)))
for route, (deferred, verdict, plain, after) in masks(overflowing, ids, edits).items():
    assert verdict, ("an overflowing seed list not reported", route)
    assert not after, ("a call without deferral leaves an overflow verdict behind", route)
    assert np.all((deferred & ~plain) == 0), ("the incomplete mask keeps a pair the complete one drops", route)
    print("OVERFLOW", route, int((deferred != 0).sum()), int((plain != 0).sum()))
for route, (deferred, verdict, plain, after) in masks(calm, ids[:2], edits[:2]).items():
    assert not verdict and not after, ("a list that fits reported as overflowed", route)
    assert np.array_equal(deferred, plain), route
    print("CALM", route, int((plain != 0).sum()))
al.close()
print("CHILD_OK")
"""

_PIPELINE = r"""
import random, sys
sys.path.insert(0, %r)
import torch
from oracle.oracle import Oracle
from porechop_amd.panel import load_panel
from porechop_amd.pipeline import Pipeline, ScanParams
from porechop_amd.synth import reads_from_strings
from tests import readgen, ref_pipeline
from tests.pairgen import mutate

panel = load_panel()
p = ScanParams()
pl = Pipeline(panel, p)
matching = [i for i, s in enumerate(panel) if s.name == "SQK-NSK007"]
middle = pl.middle_adapter_list(matching)
rng = random.Random(3)
seqs = [r[1] for r in readgen.ligation_reads(9, 120)]
for _ in range(40):                          # several middle copies per read: more seed candidates than the list holds
    body = "".join(rng.choice("ACGT") for _ in range(3000))
    for _ in range(4):
        at = rng.randint(200, 2700)
        body = body[:at] + mutate(rng, rng.choice(middle), 0.03) + body[at:]
    seqs.append(body)
reads, norm = reads_from_strings(seqs)
st, et = pl.phase_b(reads, matching)
hits = pl.phase_c(reads, st, et, matching, prefilter=True)
pl.aligner.sync()
assert pl.stats.get("prefilter_overflow_reruns", 0) >= 1, pl.stats
got = {}
for r, a, s, e in zip(hits.read.cpu().tolist(), hits.adapter.cpu().tolist(), hits.start.cpu().tolist(), hits.end.cpu().tolist()):
    got.setdefault(r, []).append((a, s, e))
stl, etl = st.cpu().tolist(), et.cpu().tolist()
oracle = Oracle()
n_hits = 0
for r, seq in enumerate(norm):
    want = [(a, s, e) for a, s, e, _ in ref_pipeline.phase_c(oracle.adapter_alignment, seq, stl[r], etl[r], pl.middle_adapters, p)]
    assert got.get(r, []) == want, (r, got.get(r), want)
    n_hits += len(want)
assert n_hits >= 100, n_hits
pl.close()
print("CHILD_OK", pl.stats["prefilter_overflow_reruns"], n_hits)
"""


def _child(code):
    r = subprocess.run([sys.executable, "-c", code % REPO], env=dict(os.environ, PC_PF_SEED_CAP="64"), capture_output=True, text=True,
                       timeout=900, cwd=REPO)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    return r


def test_deferred_verdict_reports_an_overflow_and_only_an_overflow():
    """PC_PF_SEED_CAP=64, the deferral on: an overflowing batch is reported after sync and its mask is a subset of the
    complete one; a batch that fits is not reported and its mask equals the non-deferred one exactly -- over the byte
    route and the packed route.  A call without deferral after an overflowed one resets the verdict."""
    r = _child(_VERDICT)
    assert r.stdout.count("OVERFLOW") == 2 and r.stdout.count("CALM") == 2


def test_pipeline_reruns_the_lean_prefilter_when_the_seed_list_overflows():
    """Pipeline.phase_c(prefilter=True) over byte-resident reads, one adapter set (the lean route): the deferred verdict
    says the mask is incomplete, the stage runs again without deferral, and the hits equal the reference's logic."""
    _child(_PIPELINE)
