#!/usr/bin/env python3
"""Rate probe (GPU box): the paths of the middle hits of a 100 k x 8 kb batch with 1 % chimeras through
Pipeline.middle_hit_paths (middle_path_kernel of pc_paths.hip: one lane per hit, a bounded window of the masked read), and that batch's
phase_c (the middle scan, whose code the paths do not touch), in one process, timed by device events around each call; medians
over the repeats, and their ratio.  A record, not a gate: nobody has measured this kernel before.
   python tools/middle_paths_rate.py [n_reads] [repeats]        (default 100 000, 5)"""
import statistics
import sys
sys.path.insert(0, ".")
import torch
from porechop_amd.panel import load_panel
from porechop_amd.pipeline import Pipeline, ScanParams
from porechop_amd.synth import make_reads

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
pl = Pipeline(load_panel(), ScanParams())
reads = make_reads(n, 8000, seed=3, start_frac=0.9, end_frac=0.5, chimera_frac=0.01)
bs, be = pl.phase_a(reads, torch.arange(min(n, 10_000), device="cuda"))
matching = pl.matching_sets(bs, be)
st, et = pl.phase_b(reads, matching)
pl.aligner.sync()


def timed(fn):
    ms = []
    for _ in range(reps + 1):                       # (the first run allocates scratch: dropped)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        pl.aligner.sync()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[1:]), ms[1:], res


t_c, all_c, hits = timed(lambda: pl.phase_c(reads, st, et, matching, prefilter=True))
t_p, all_p, (recs, heads, ops) = timed(lambda: pl.middle_hit_paths(reads, st, et, hits))
H = int(hits.read.numel())
per_read = torch.bincount(torch.bincount(hits.read)).tolist() if H else []
cols = pl.aligner.middle_paths_cols(8000)
print("device: %s   reads: %d x 8000 bases, 1 %% chimeras   middle adapters: %d   repeats: %d"
      % (torch.cuda.get_device_name(0), n, len(pl.middle_adapters), reps))
print("middle hits: %d in %d rounds   reads by hit count (0, 1, 2, ...): %s   widest window: %d columns" % (H, hits.rounds, per_read, cols))
print("phase_c (prefilter route) : median %.3f ms  (%s)" % (t_c, " ".join("%.3f" % x for x in all_c)))
print("middle_hit_paths          : median %.3f ms  (%s)  %.3f M hits/s   path steps returned: %d"
      % (t_p, " ".join("%.3f" % x for x in all_p), H / t_p / 1e3 if t_p else 0.0, int(heads[:, 0].sum())))
print("ratio middle_hit_paths / phase_c: %.3f" % (t_p / t_c))
pl.close()
