#!/usr/bin/env python3
"""What a pc_scan_device call costs when its table has to be planned: a phase A job list (every start / end sequence of the
panel over the same end windows, MODE_TRACE) alternating with one that is 64 windows shorter, so that no call finds the
cached table.  bench.py's steps repeat one job list and never see this.
usage: time_replan.py [windows [calls]]  ->  one line: ms per call (wall clock over `calls` calls, synchronised at the end)"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from porechop_amd.batch import MODE_TRACE, Aligner  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
with open(os.path.join(REPO, "tests", "golden", "panel.json")) as f:
    seqs = sorted({x[1] for a in json.load(f) for x in (a["start"], a["end"]) if x})
dev = torch.device("cuda", 0)
g = torch.Generator(device="cpu").manual_seed(5)
arena = torch.from_numpy(np.frombuffer(b"ACGT", dtype=np.uint8).copy())[torch.randint(0, 4, (n * 150 + 256,), generator=g)].to(dev)
off = (torch.arange(n, dtype=torch.int64) * 150).to(dev)
length = torch.full((n,), 150, dtype=torch.int32, device=dev)
k = len(seqs)
al = Aligner(seqs)
lists = []
for m in (n, n - 64):       # every job over windows [0, m)
    lists.append((off[:m].repeat(k), length[:m].repeat(k), np.arange(k, dtype=np.int32), np.arange(k + 1, dtype=np.int64) * m,
                  torch.zeros((k * m, 8), dtype=torch.int32, device=dev)))


def run(count):
    for i in range(count):
        wo, wl, ja, js, out = lists[i & 1]
        al.scan_device(arena, wo, wl, ja, js, 150, out, MODE_TRACE)
    al.sync()
    torch.cuda.synchronize()


run(20)
t0 = time.perf_counter()
run(calls)
dt = time.perf_counter() - t0
print("REPLAN jobs %d windows %d calls %d ms_per_call %.4f" % (k, n, calls, 1e3 * dt / calls))
al.close()
