"""The prefilter's cached plan (pc_prefilter_plan.h, uploaded by pc_api.cpp) when one Aligner is asked for other adapter lists,
bounds and routes in turn: every call's mask is the mask a fresh Aligner gives for that single call -- nothing of the list
before survives in the tables, launch lists or seed-stage scalars -- and the byte route's is the oracle's."""
import random

import numpy as np
import pytest
import torch

from tests.pairgen import mutate
from tests.test_gpu_packed_total import Batch, Y_BOTTOM, Y_TOP, bits_of

pytestmark = pytest.mark.gpu


def test_each_call_gets_the_mask_of_a_fresh_aligner(oracle):
    import porechop_amd
    rng = random.Random(11)
    seq = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    panel = [Y_TOP, Y_BOTTOM, seq(24), seq(10), seq(30), seq(32),            # 0..5: at most 32 bases
             "ACGTNNACGTTTGACCAGTNAC", seq(40)]                              # 6: with N; 7: 40 bases
    list_a, list_b, list_c = [0, 1, 2, 3, 4, 5], [0, 1, 2], [6, 7, 0]
    # 64 windows of 1100 bases (three column chunks), copies with 0..15 % edits anywhere, the chunk borders included
    reads = []
    for i in range(64):
        r = list(seq(1100))
        for s in ([rng.randrange(1060)] + [368 * (1 + i % 2) - rng.randrange(30)]):
            mut = mutate(rng, panel[rng.randrange(len(panel))].replace("N", "A"), rng.choice([0.0, 0.05, 0.1, 0.15]))
            r[s:s + len(mut)] = mut
        reads.append("".join(r)[:1100])
    assert set("".join(reads)) <= set("ACGT")
    b = Batch(reads, torch.device("cuda"))

    def call(al, route, ids, thr):
        ks = [al.max_edits(len(panel[j]), thr) for j in ids]
        if route == "bytes":
            m = al.prefilter_mask(b.arena, b.d_off, b.d_len, b.max_len, ids, ks)
        else:
            m = al.prefilter_mask_packed(b.plane, b.d_off, b.d_len, b.max_len, ids, ks, total=(route == "plane_total"))
        al.sync()
        assert m is not None, (route, ids, thr)
        return m.cpu().numpy(), ks

    calls = [("bytes", list_a, 90.0), ("plane_total", list_a, 90.0), ("plane_seeds", list_b, 90.0), ("bytes", list_a, 80.0),
             ("plane_total", list_c, 85.0), ("bytes", list_a, 90.0)]
    dist = {j: oracle.min_edits_many(b.arr, b.offs, b.lens, panel[j]) for j in list_a}
    al = porechop_amd.Aligner(panel)
    try:
        for n, (route, ids, thr) in enumerate(calls):
            got, ks = call(al, route, ids, thr)
            fresh = porechop_amd.Aligner(panel)
            try:
                want, _ = call(fresh, route, ids, thr)
            finally:
                fresh.close()
            assert np.array_equal(got, want), (n, route, ids, thr, int((got != want).sum()))
            assert (got != 0).any() and not bits_of(got, len(ids)).all()
            if route == "bytes":
                bits = bits_of(got, len(ids))
                for col, (j, k) in enumerate(zip(ids, ks)):
                    assert np.array_equal(bits[col], dist[j] <= k), (n, j, k)
    finally:
        al.close()
