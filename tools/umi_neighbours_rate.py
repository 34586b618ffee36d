#!/usr/bin/env python3
"""Rate probe (GPU box) of the UMI neighbours kernel (umi_neighbours_kernel of pc_umi_groups.hip): n keys,
5 % of them copies of other keys at 1 .. 3 edits, max_dist 2, all against all, in one process, timed by device events around
pc_umi_neighbours itself, five alternating repetitions of
   key length 22 (the 32-bit kernel) and 44 (the 64-bit kernel), each with the prunes on -- the keys as they come (shuffled) and
   in umi_groups.kernel_order (by length, then composition: the order the run hands them in) -- and with PC_UMI_NO_PRUNE=1.
Medians with their spread; pairs per second; DP columns per second (without the prunes every pair runs every column of its
text key); the share of pairs the lower bound settles (counted in torch over 1 024 sampled keys against all others); the time
at 2^20 keys, extrapolated by the pair count; and the only baseline there is: umi_groups.neighbours_host (numpy) on a sample of
4 096 keys on the same box.  A record, not a gate.
   python tools/umi_neighbours_rate.py [n_keys] [repeats] [host_sample] [out.txt]     (default 65 536, 5, 4 096, profiles/umi_neighbours_rate.txt)"""
import ctypes
import os
import random
import statistics
import sys
import time
sys.path.insert(0, ".")
import numpy as np
import torch
import porechop_amd
from porechop_amd import umi_groups as ug

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
host_n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
out_path = sys.argv[4] if len(sys.argv) > 4 else "profiles/umi_neighbours_rate.txt"
MAX_DIST = 2
CAP = 1 << 22
dev = torch.device("cuda")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_keys(length, seed):
    rng = random.Random(seed)
    keys = ["".join(rng.choice("ACGT") for _ in range(length)) for _ in range(n - n // 20)]
    while len(keys) < n:
        k = list(keys[rng.randrange(n - n // 20)])
        for _ in range(rng.randrange(1, 4)):
            kind, at = rng.randrange(3), rng.randrange(len(k))
            if kind == 0:
                k[at] = rng.choice("ACGT")
            elif kind == 1:
                k.insert(at, rng.choice("ACGT"))
            else:
                del k[at]
        keys.append("".join(k))
    rng.shuffle(keys)
    return keys


def settled_share(planes, lens):
    """The share of pairs whose lower bound is above MAX_DIST, over 1 024 sampled keys against all keys."""
    p = torch.from_numpy(planes.view(np.int64)).to(dev)
    ln = torch.from_numpy(lens.astype(np.int64)).to(dev)
    bits = ((p[:, :, None] >> torch.arange(64, device=dev)[None, None, :]) & 1) * (torch.arange(64, device=dev)[None, None, :] < ln[:, None, None])
    code = bits[:, 0, :] + 2 * bits[:, 1, :]
    inside = torch.arange(64, device=dev)[None, :] < ln[:, None]
    comp = torch.stack([((code == c) & inside).sum(1) for c in range(4)], dim=1)            # [n, 4]
    rows = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:1024]
    sad = (comp[rows][:, None, :] - comp[None, :, :]).abs().sum(2)
    bound = (sad + (ln[rows][:, None] - ln[None, :]).abs()) // 2
    return float((bound > MAX_DIST).float().mean().item())


al = porechop_amd.Aligner(["ACGTACGTACGT"])
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
pairs = torch.empty((CAP, 3), dtype=torch.int32, device=dev)
found = torch.zeros(1, dtype=torch.int64, device=dev)
sets = {}
for length in (22, 44):
    planes, lens = ug.pack(make_keys(length, length))
    order = ug.kernel_order(planes, lens)
    sets[length] = (planes, lens, torch.from_numpy(planes.view(np.int64)).to(dev), torch.from_numpy(lens).to(dev), int(lens.max()),
                    torch.from_numpy(np.ascontiguousarray(planes[order]).view(np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(lens[order])).to(dev))


def once(length, no_prune, ordered):
    _, _, p, ln, max_len, po, lo = sets[length]
    if ordered:
        p, ln = po, lo
    if no_prune:
        os.environ["PC_UMI_NO_PRUNE"] = "1"
    else:
        os.environ.pop("PC_UMI_NO_PRUNE", None)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = al.lib.pc_umi_neighbours(al._ctx, p.data_ptr(), ln.data_ptr(), n, max_len, MAX_DIST, pairs.data_ptr(), CAP, found.data_ptr(), stream)
    e1.record()
    assert rc == 0
    al.sync()
    return e0.elapsed_time(e1), int(found.item())


configs = [(22, False, False), (22, False, True), (22, True, False), (44, False, False), (44, False, True), (44, True, False)]
ms = {c: [] for c in configs}
count = {}
for rep in range(reps + 1):                         # (the first round is a warm-up: dropped)
    for c in configs:
        t, m = once(*c)
        count.setdefault(c, m)
        assert count[c] == m
        if rep:
            ms[c].append(t)
os.environ.pop("PC_UMI_NO_PRUNE", None)
for length in (22, 44):
    assert count[(length, False, False)] == count[(length, False, True)] == count[(length, True, False)]

all_pairs = n * (n - 1) // 2
big = (1 << 20) * ((1 << 20) - 1) // 2
say("device: %s   keys: %d (5 %% copies at 1..3 edits)   max_dist: %d   pairs: %d   repeats: %d (alternating)"
    % (torch.cuda.get_device_name(0), n, MAX_DIST, all_pairs, reps))
for length, no_prune, ordered in configs:
    v = ms[(length, no_prune, ordered)]
    med = statistics.median(v)
    planes, lens = sets[length][0], sets[length][1]
    text = "length %d (%d-bit kernel), %s: median %.3f ms  (%s; spread %.3f)  found %d  %.1f G pairs/s" % (
        length, 32 if sets[length][4] <= 32 else 64, "no prune" if no_prune else ("prunes on, kernel_order" if ordered else "prunes on, shuffled"), med, " ".join("%.3f" % x for x in v),
        max(v) - min(v), count[(length, no_prune, ordered)], all_pairs / med / 1e6)
    if no_prune:
        cols = float(lens.astype(np.int64).sum()) * (n - 1) / 2              # every pair runs the columns of one of its two keys
        text += "  %.1f G DP columns/s" % (cols / med / 1e6)
    else:
        text += "  lower bound settles %.1f %% of the pairs" % (100 * settled_share(planes, lens))
    text += "  -> 2^20 keys: %.2f s" % (med / 1e3 * big / all_pairs)
    say(text)
for length in (22, 44):
    planes, lens = sets[length][0][:host_n], sets[length][1][:host_n]
    t0 = time.perf_counter()
    got = ug.neighbours_host(planes, lens, MAX_DIST)
    dt = time.perf_counter() - t0
    hp = host_n * (host_n - 1) // 2
    say("length %d, neighbours_host (numpy, one core) on %d keys: %.2f s  found %d  %.2f M pairs/s   the kernel in kernel_order: %.0f x"
        % (length, host_n, dt, got.shape[0], hp / dt / 1e6, (all_pairs / statistics.median(ms[(length, False, True)]) * 1e3) / (hp / dt)))
al.close()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
