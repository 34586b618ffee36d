#!/usr/bin/env python3
"""What the explain route costs on the barcoded phase-B step (GPU box): the same 1 M reads, 98 matching sets (196 jobs),
timed three ways in ONE process, alternating, after warm-up --
  explain   every pair traced + pc_phase_b_explain (both passes) + pc_phase_b_reduce for the call   Pipeline.phase_b_explain
  traced    every pair traced + pc_phase_b_reduce                                                   phase_b_demux(prune=False)
  pruned    the exact pruning, the default of a run without a report (unchanged by the explain route) phase_b_demux(prune=True)
and the explain pass alone on resident records (summary pass, prefix sum, fill pass).  Times are host clocks around work that
ends in a device synchronise; median and range over the repetitions.  Results of the three are compared before timing.
    python tools/explain_overhead.py [n_reads] [read_len] [reps] > profiles/explain_overhead.txt"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from porechop_amd import panel as rules
from porechop_amd.panel import load_panel
from porechop_amd.pipeline import MODE_TRACE, Pipeline, ScanParams
from porechop_amd.runner import barcode_bins
from porechop_amd.synth import make_reads

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
read_len = int(sys.argv[2]) if len(sys.argv) > 2 else 8000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"
panel = load_panel()
fw = [s for s in panel if s.name.startswith("Barcode ") and "(forward)" in s.name]
pl = Pipeline(panel, ScanParams())
p = pl.p
reads = make_reads(n, read_len, seed=2, barcodes_start=[s.start[1] for s in fw], barcodes_end=[s.end[1] for s in fw])
matching = [i for i, s in enumerate(pl.sets) if s.name == "SQK-NSK007" or s in fw]
names, bins = barcode_bins(pl, [i for i in matching if rules.is_barcode(pl.sets[i])])
jobs, where = pl._phase_b_jobs(reads, matching)
J = len(jobs)


def sync():
    pl.aligner.sync()
    torch.cuda.synchronize()
    return time.perf_counter()


routes = {
    "explain": lambda: pl.phase_b_explain(reads, matching, bins, 75.0, 5.0, False)[:3],
    "traced": lambda: pl.phase_b_demux(reads, matching, bins, 75.0, 5.0, False, prune=False),
    "pruned": lambda: pl.phase_b_demux(reads, matching, bins, 75.0, 5.0, False, prune=True),
}
# same answers first (and the warm-up of every shape)
ref = None
for _ in range(2):
    for name, fn in routes.items():
        st, et, call = fn()
        sync()
        if ref is None:
            ref = (st.clone(), et.clone(), call.copy())
        assert torch.equal(st, ref[0]) and torch.equal(et, ref[1]) and np.array_equal(call, ref[2]), name
times = {k: [] for k in routes}
for _ in range(reps):
    for name, fn in routes.items():
        t0 = sync()
        fn()
        times[name].append((sync() - t0) * 1e3)
# the pass alone, on resident records
_, rec, rec_off = pl._scan_jobs(pl._ends_arena(reads), jobs, MODE_TRACE, p.end_size, with_layout=True)
sides = [w[0] for w in where]
job_of = {(si, side): k for k, (side, si) in enumerate(where)}
jb = [(job_of.get((b[0], 0), -1), job_of.get((b[1], 1), -1)) for b in bins]
alone, red = [], []
rows = 0
for k in range(reps + 2):
    t0 = sync()
    out = pl.aligner.phase_b_explain(rec, n, rec_off, sides, p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold, bins=jb)
    t1 = sync()
    a = torch.zeros(n, dtype=torch.int32, device="cuda"); b = torch.zeros_like(a); c = torch.zeros_like(a)
    t2 = sync()
    pl.aligner.phase_b_reduce(rec, n, rec_off, sides, p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold, a, b, bins=jb,
                              barcode_threshold=75.0, barcode_diff=5.0, require_two=False, call=c)
    t3 = sync()
    rows = int(out[3].shape[0])
    if k >= 2:
        alone.append((t1 - t0) * 1e3)
        red.append((t3 - t2) * 1e3)
rec_bytes = J * n * 32
out_bytes = n * (48 + 32 + 8) + rows * 24
fmt = lambda xs: "median %8.2f ms  (min %8.2f, max %8.2f, %d reps)" % (statistics.median(xs), min(xs), max(xs), len(xs))
print("explain overhead: %d reads x %d bases, %d jobs (%d sets), %d bins; %s" % (n, read_len, J, len(matching), len(bins), torch.cuda.get_device_name(0)))
for name in routes:
    print("  phase B, %-8s %s" % (name + ":", fmt(times[name])))
me, mt, mp = (statistics.median(times[k]) for k in ("explain", "traced", "pruned"))
print("  explain over traced: %+.2f ms (%+.1f %%); explain over pruned: %.2fx" % (me - mt, 100.0 * (me - mt) / mt, me / mp))
print("  the explain pass alone (summary, prefix sum + its total to the host, fill): %s" % fmt(alone))
print("  pc_phase_b_reduce on the same records:                                     %s" % fmt(red))
print("  bytes: records %.2f GB read by the summary pass and again by the fill pass; %d qualifying alignments, %.3f GB written"
      % (rec_bytes / 1e9, rows, out_bytes / 1e9))
print("  achieved over the two passes: %.2f TB/s of record reads" % (2 * rec_bytes / 1e9 / statistics.median(alone)))
pl.close()
