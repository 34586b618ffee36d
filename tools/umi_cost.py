#!/usr/bin/env python3
"""Cost probe (GPU box) of the UMI kernel (umi_kernel of pc_paths.hip): 1 M end windows x 150 columns, each with
a copy of the 28-row UMI adapter TTTVVVVTTVVVVTTVVVVTTVVVVTTT, in one process, timed by device events around each call, five
alternating repetitions:
   (a) Aligner.align_paths   a table that holds only that adapter (path_kernel: the operations leave the device)
   (b) Aligner.umis          the same table (umi_kernel: the operations stay in a scratch, one walk more)
   (c) Aligner.umis          the built-in panel in front of the adapter (the LDS and the scratch are the CALL's adapter's)
Medians, the spread of (a)'s own repetitions, and the ratios (b)/(a) and (c)/(b).  A record, not a gate.
   python tools/umi_cost.py [n_windows] [repeats]        (default 1 000 000, 5)"""
import statistics
import sys
sys.path.insert(0, ".")
import torch
import porechop_amd
from porechop_amd.panel import load_panel

UMI28 = "TTTVVVVTTVVVVTTVVVVTTVVVVTTT"
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda")
g = torch.Generator(device=dev)
g.manual_seed(28)
letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
arena = letters[torch.randint(0, 4, (n, 150), device=dev, generator=g)]
inst = torch.where(torch.tensor([c == "V" for c in UMI28], device=dev)[None, :],
                   letters[torch.randint(0, 3, (n, 28), device=dev, generator=g)], torch.full((n, 28), ord("T"), dtype=torch.uint8, device=dev))
at = torch.randint(0, 150 - 28 + 1, (n, 1), device=dev, generator=g)
arena.scatter_(1, at + torch.arange(28, device=dev)[None, :], inst)
arena = torch.cat([arena.reshape(-1), torch.full((64,), ord("N"), dtype=torch.uint8, device=dev)])
off = torch.arange(n, dtype=torch.int64, device=dev) * 150
length = torch.full((n,), 150, dtype=torch.int32, device=dev)

alone = porechop_amd.Aligner([UMI28], wildcards=True)
seqs = []
for s in load_panel():
    for side in (s.start, s.end):
        if side is not None and side[1] not in seqs:
            seqs.append(side[1])
behind = porechop_amd.Aligner(seqs + [UMI28], wildcards=True)
idx0 = torch.zeros(n, dtype=torch.int32, device=dev)


def once(al, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    al.sync()
    return e0.elapsed_time(e1), res


calls = {"a": (alone, lambda: alone.align_paths(arena, off, length, idx0, max_len=150)),
         "b": (alone, lambda: alone.umis(arena, off, length, 0, 0, max_len=150)),
         "c": (behind, lambda: behind.umis(arena, off, length, len(seqs), 0, max_len=150))}
ms = {k: [] for k in calls}
out = {}
for rep in range(reps + 1):                         # (the first round allocates the scratch: dropped)
    for k, (al, fn) in calls.items():
        t, out[k] = once(al, fn)
        if rep:
            ms[k].append(t)
med = {k: statistics.median(v) for k, v in ms.items()}
spread = max(ms["a"]) - min(ms["a"])
same = bool((out["a"][0] == out["b"][0]).all()) and bool((out["b"][0] == out["c"][0]).all()) and bool((out["b"][1] == out["c"][1]).all())
status = torch.bincount(out["b"][1][:, 0], minlength=4).tolist()
print("device: %s   windows: %d x 150 bases x one 28-row UMI adapter   repeats: %d (alternating)   longest adapter of the panel: %d rows"
      % (torch.cuda.get_device_name(0), n, reps, max(len(x) for x in seqs)))
for k, what in (("a", "align_paths, table of one      "), ("b", "umis, table of one             "), ("c", "umis, behind the built-in panel")):
    print("(%s) %s: median %.3f ms  (%s)  %.2f M windows/s" % (k, what, med[k], " ".join("%.3f" % x for x in ms[k]), n / med[k] / 1e3))
print("spread of (a): %.3f ms   (b) - (a): %+.3f ms   (b)/(a): %.3f   (c) - (b): %+.3f ms   (c)/(b): %.3f"
      % (spread, med["b"] - med["a"], med["b"] / med["a"], med["c"] - med["b"], med["c"] / med["b"]))
print("records and UMIs identical across the three: %s   statuses 0..3: %s" % (same, status))
alone.close()
behind.close()
