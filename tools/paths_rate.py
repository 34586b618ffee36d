#!/usr/bin/env python3
"""Rate probe (GPU box): N end windows of 150 bases against one 28-mer through Aligner.align_paths (the plain-int32 path
kernel, pc_paths.hip) and through the MODE_TRACE scan of the same pairs (the packed traced kernel), in one process, timed by
device events around each call; medians over the repeats, and their ratio.  The records of the two are compared on the way.
   python tools/paths_rate.py [n_windows] [repeats]        (default 1 000 000, 5)"""
import statistics
import sys
sys.path.insert(0, ".")
import torch
import porechop_amd

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, AD = 150, "AATGTACTTCGTTCAGTTACGTATTGCT"
g = torch.Generator(device="cuda").manual_seed(5)
letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
arena = letters[torch.randint(0, 4, (n * W + 64,), device="cuda", generator=g)]
# nine windows in ten carry the adapter, one base in twelve of it redrawn
rows = torch.nonzero(torch.rand(n, device="cuda", generator=g) < 0.9).flatten()
at = rows * W + torch.randint(0, W - len(AD), (rows.shape[0],), device="cuda", generator=g)
copy = torch.tensor(list(AD.encode()), dtype=torch.uint8, device="cuda")[None, :].repeat(rows.shape[0], 1)
redraw = torch.rand(copy.shape, device="cuda", generator=g) < 1.0 / 12
copy[redraw] = letters[torch.randint(0, 4, (int(redraw.sum()),), device="cuda", generator=g)]
arena[(at[:, None] + torch.arange(len(AD), device="cuda")[None, :]).flatten()] = copy.flatten()
off = torch.arange(n, dtype=torch.int64, device="cuda") * W
wl = torch.full((n,), W, dtype=torch.int32, device="cuda")
idx = torch.zeros(n, dtype=torch.int32, device="cuda")
out = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
al = porechop_amd.Aligner([AD])


def timed(fn):
    ms = []
    for _ in range(reps + 1):                       # (the first run allocates scratch: dropped)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        al.sync()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[1:]), ms[1:], res


t_scan, all_scan, _ = timed(lambda: al.scan_device(arena, off, wl, [0], [0, n], W, out, porechop_amd.MODE_TRACE))
t_path, all_path, (recs, heads, ops) = timed(lambda: al.align_paths(arena, off, wl, idx, max_len=W))
same = bool((recs == out).all())
steps = int(heads[:, 0].sum())
cells = n * W * len(AD)
print("device: %s   windows: %d x %d bases x one %d-mer   repeats: %d" % (torch.cuda.get_device_name(0), n, W, len(AD), reps))
print("MODE_TRACE scan : median %.3f ms  (%s)  %.1f Gcells/s" % (t_scan, " ".join("%.3f" % x for x in all_scan), cells / t_scan / 1e6))
print("align_paths     : median %.3f ms  (%s)  %.1f Gcells/s  %.2f M pairs/s" % (t_path, " ".join("%.3f" % x for x in all_path),
                                                                              cells / t_path / 1e6, n / t_path / 1e3))
print("ratio align_paths / scan: %.1f   records identical: %s   path steps returned: %d" % (t_path / t_scan, same, steps))
al.close()
sys.exit(0 if same else 1)
