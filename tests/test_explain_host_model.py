"""tests/explain_ref.py -- the host restatement the HIP kernel is tested against (tests/test_gpu_explain.py) -- checked
itself: against the line-for-line mirror of the reference's per-read logic (tests/ref_pipeline.py) on records the oracle
aligned, and Pipeline's torch formulation (the route of aligners without the kernel) against it on generated tables."""
import random

import numpy as np
import torch

from tests import explain_ref, explaingen, readgen, ref_pipeline

END = 150


def test_host_model_equals_the_sequential_reference_logic(oracle):
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import ScanParams
    by_name = {s.name: s for s in load_panel()}
    sets = [by_name["SQK-NSK007"]] + [by_name["Barcode %d (reverse)" % k] for k in (1, 2, 3, 7, 9)]
    matching = list(range(len(sets)))
    seqs = [s.upper().replace("U", "T") for _, s, _ in readgen.native_reads(11, 70)] + ["", "A"]
    R = len(seqs)
    assert any(len(s) < END for s in seqs)
    for scores, end_threshold, min_trim in (((3, -6, -5, -2), 75.0, 4), ((2, -3, -5, -2), 60.0, 12)):
        p = ScanParams(scores=scores, end_threshold=end_threshold, min_trim_size=min_trim)
        jobs = [(side, si) for si in matching for side in (0, 1)]            # phase B's job order: set by set, start then end
        recs = np.zeros((len(jobs) * R, 8), dtype=np.int32)
        offs = [j * R for j in range(len(jobs))]
        for j, (side, si) in enumerate(jobs):
            ad = sets[si].end[1] if side else sets[si].start[1]
            for r, s in enumerate(seqs):
                res = oracle.align_raw(s[-END:] if side else s[:END], ad, scores)
                recs[offs[j] + r] = [-1, 0, -1, 0, -2147483648, 0, 0, 0] if res.failed else \
                    [res.read_start, res.read_end, res.adapter_start, res.adapter_end, res.score, res.aligned_matches, res.aligned_len, res.full_len]
        names = [ref_pipeline.barcode_name(s) for s in sets[1:]]
        job_of = {js: j for j, js in enumerate(jobs)}
        bins = [(job_of[(0, si)], job_of[(1, si)]) for si in matching[1:]]
        summary, bscore, hit_first, hits = explain_ref.explain(recs, R, offs, [j[0] for j in jobs], END, p.min_trim_size, p.extra_end_trim,
                                                               p.end_threshold, bins)
        fn = lambda rd, ad, sc: oracle.adapter_alignment(rd, ad, sc)
        listed = called = 0
        for r, seq in enumerate(seqs):
            st, et, s_sc, e_sc = ref_pipeline.phase_b_barcodes(fn, seq, sets, matching, p, "reverse")
            assert (st, et) == tuple(summary[r, 0:2]), r
            # the reference's two lists (nanopore_read.py:178-183,200-205), rebuilt from the same calls
            want = []
            for side in (0, 1):
                for si in matching:
                    ad = sets[si].end[1] if side else sets[si].start[1]
                    full, partial, rs, re = ref_pipeline.align_adapter(fn, seq[-END:] if side else seq[:END], ad, scores)
                    edge = rs != 0 if side else re != END
                    if partial > p.end_threshold and edge and re - rs >= p.min_trim_size:
                        want.append((job_of[(side, si)], rs, re, full, partial))
            got = [(j, rs, re, explain_ref.record_fields([[0, 0, 0, 0, 0, m, al, fl]])[0][0], explain_ref.record_fields([[0, 0, 0, 0, 0, m, al, fl]])[0][1])
                   for j, rs, re, m, al, fl in hits[hit_first[r]:hit_first[r + 1]].tolist()]
            assert got == want, (r, got, want)
            listed += len(want)
            for col, sc in ((0, s_sc), (1, e_sc)):
                ranked = sorted(sc.items(), reverse=True, key=lambda x: x[1])
                for rank in range(2):
                    name, v = ranked[rank] if len(ranked) > rank else ("none", 0.0)
                    k = int(summary[r, 6 + 2 * col + rank])
                    assert ((names[k] if k >= 0 else "none"), float(bscore[r, 2 * col + rank])) == (name, v), (r, col, rank)
            for thr, diff, two in ((75.0, 5.0, False), (75.0, 5.0, True), (60.0, 0.0, False)):
                k = explain_ref.implied_call(summary[r], bscore[r], thr, diff, two)
                want_call = ref_pipeline.determine_barcode(s_sc, e_sc, thr, diff, two)
                assert (names[k] if k >= 0 else "none") == want_call, (r, thr, diff, two)
                called += want_call != "none"
        assert listed > R and called > R // 2


def test_torch_formulation_equals_the_host_model():
    from porechop_amd.pipeline import Pipeline, ScanParams

    class NoAligner:
        def set_adapters(self, adapters):
            pass
    checked = ties = 0
    for seed, (n, J, nbins, shared) in enumerate([(1, 1, 0, False), (65, 4, 2, False), (257, 9, 4, False), (130, 12, 5, True), (64, 24, 12, False)]):
        rng = np.random.default_rng(100 + seed)
        recs, offs, sides, bins = explaingen.case(rng, n, J, nbins, shared_jobs=shared)
        for end_threshold, min_trim, extra in ((75.0, 50, 2), (33.333333, 51, 0), (0.0, 1, 7)):
            pl = Pipeline([], ScanParams(end_threshold=end_threshold, min_trim_size=min_trim, extra_end_trim=extra), aligner=NoAligner())
            want = explain_ref.explain(recs, n, offs, sides, END, min_trim, extra, end_threshold, bins)
            rec = torch.from_numpy(np.stack([recs[o:o + n] for o in offs]))
            got = pl._explain_torch(rec, [int(s) for s in sides], bins)
            for name, g, w in zip(("summary", "bscore", "hit_first", "hits"), got, want):
                assert np.array_equal(g.numpy(), w), (seed, name, end_threshold)
            checked += n
            s = want[0]
            ties += int(((s[:, 2] >= 2) | (s[:, 3] >= 2)).sum())
            if nbins >= 2:
                ties += int((want[1][:, 0] == want[1][:, 1]).sum())
    assert checked > 1000 and ties > 50
