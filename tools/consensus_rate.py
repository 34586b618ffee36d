#!/usr/bin/env python3
"""Rate probe (GPU box) of the UMI consensus round (consensus_pileup_kernel + consensus_call_kernel of pc_consensus.hip, DESIGN.md
section 18): `groups` groups of 8 members, copies of an 8 192-base original at 6 % errors (2 % substitutions, 2 % insertions, 2 %
deletions), round 1 (the first member is the template, the other seven are aligned to it), in one process, timed by device events
around pc_consensus_round itself, five alternating repetitions of band 64 (three cells to a lane) and band 32 (two).  Medians
with their spread; band cells per second (pairs x template rows x (2 band + 1)); groups per second; the slices the call was cut
into under PC_CONSENSUS_SCRATCH_MB (default 4 096); and the only baseline there is: consensus.round_host (numpy) on one core of the
same box over `host_groups` of those groups, which must give the same bytes.  A record, not a gate.
   python tools/consensus_rate.py [groups] [repeats] [host_groups] [out.txt]     (default 4 096, 5, 16, profiles/consensus_rate.txt)"""
import ctypes
import os
import statistics
import sys
import time
sys.path.insert(0, ".")
import numpy as np
import torch
import porechop_amd
from porechop_amd import consensus as cs

G = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
host_g = int(sys.argv[3]) if len(sys.argv) > 3 else 16
out_path = sys.argv[4] if len(sys.argv) > 4 else "profiles/consensus_rate.txt"
COPIES, LENGTH, RATE = 8, 8192, 0.02
dev = torch.device("cuda")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def copy_of(rng, orig):
    r = rng.random(orig.size)
    bases = np.where(r < RATE, (orig + rng.integers(1, 4, orig.size)) % 4, orig)
    deleted = (r >= RATE) & (r < 2 * RATE)
    inserted = (r >= 2 * RATE) & (r < 3 * RATE)
    counts = np.where(deleted, 0, np.where(inserted, 2, 1))
    out = np.repeat(bases, counts)
    starts = np.cumsum(counts) - counts
    out[starts[inserted]] = rng.integers(0, 4, int(inserted.sum()))
    return out


t0 = time.time()
rng = np.random.default_rng(1818)
letters = np.frombuffer(b"ACGT", dtype=np.uint8)
seqs = []
for g in range(G):
    orig = rng.integers(0, 4, LENGTH)
    seqs += [letters[copy_of(rng, orig)] for _ in range(COPIES)]
lens = np.array([s.size for s in seqs], dtype=np.int64)
off = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)
arena_h = np.concatenate(seqs + [np.zeros(64, dtype=np.uint8)])
say("%d groups x %d members, copies of %d-base originals at %.0f %% errors: %.1f MB of reads, made in %.1f s" % (
    G, COPIES, LENGTH, 300 * RATE, arena_h.size / 1e6, time.time() - t0))

tmpl_idx = np.arange(G) * COPIES
member_idx = np.array([g * COPIES + k for g in range(G) for k in range(1, COPIES)], dtype=np.int64)
tmpl_off, tmpl_len = off[tmpl_idx].copy(), lens[tmpl_idx].astype(np.int32)
member_off, member_len = off[member_idx].copy(), lens[member_idx].astype(np.int32)
member_group = np.repeat(np.arange(G, dtype=np.int32), COPIES - 1)
first = (np.arange(G + 1, dtype=np.int64) * (COPIES - 1)).copy()
M = member_idx.size

al = porechop_amd.Aligner(["ACGTACGTACGT"])
arena = torch.from_numpy(arena_h).to(dev)
d_off, d_len, d_grp = (torch.from_numpy(x).to(dev) for x in (member_off, member_len, member_group))
cons_off = np.concatenate([[0], np.cumsum(cs.cons_capacity(tmpl_len.astype(np.int64)))])
cons = torch.empty(int(cons_off[-1]) + 16, dtype=torch.uint8, device=dev)
d_lens = torch.zeros(G, dtype=torch.int32, device=dev)
voters = torch.zeros(G, dtype=torch.int32, device=dev)
out = torch.zeros((M, 2), dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream


def run(band):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    rc = al.lib.pc_consensus_round(al._ctx, arena.data_ptr(), arena.data_ptr(), tmpl_off.ctypes.data, tmpl_len.ctypes.data, first.ctypes.data, G,
                                   d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), M, band, 30, 65535, 1, cons.data_ptr(), d_lens.data_ptr(),
                                   voters.data_ptr(), out.data_ptr(), None, None, ctypes.c_void_p(stream))
    assert rc == 0, rc
    stop.record()
    al.sync()
    return start.elapsed_time(stop)


run(64), run(32)                                           # warm-up: the scratch is allocated here
ms = {64: [], 32: []}
for _ in range(reps):
    for band in (64, 32):
        ms[band].append(run(band))
rows = float(tmpl_len[member_group].astype(np.int64).sum())
per_group = float(np.mean(4 * cs.votes_per_group(tmpl_len.astype(np.int64)) + (COPIES - 1) * (tmpl_len.astype(np.int64).max() + 1) * 64))
BUDGET_MB = int(os.environ.get("PC_CONSENSUS_SCRATCH_MB", "4096"))
say("scratch per group about %.2f MB (votes + trace): about %d slices of %d groups under PC_CONSENSUS_SCRATCH_MB = %d" % (
    per_group / 2**20, -(-G // max(1, int((BUDGET_MB << 20) // per_group))), min(G, int((BUDGET_MB << 20) // per_group)), BUDGET_MB))
for band in (64, 32):
    med = statistics.median(ms[band])
    cells = rows * (2 * band + 1)
    say("band %3d: %8.1f ms median of %d (min %.1f, max %.1f)   %.3f T band cells/s   %.0f groups/s   %.0f pairs/s" % (
        band, med, reps, min(ms[band]), max(ms[band]), cells / med / 1e9, G / med * 1e3, M / med * 1e3))
run(64)
status = out.cpu().numpy()
h_lens = d_lens.cpu().numpy()
say("band 64: %d of %d members accepted; consensus lengths %d .. %d" % (int((status[:, 0] == 0).sum()), M, int(h_lens.min()), int(h_lens.max())))

if host_g:
    hg = min(host_g, G)
    t0 = time.perf_counter()
    want = cs.round_host([seqs[g * COPIES].tobytes() for g in range(hg)], [seqs[m].tobytes() for m in member_idx[:hg * (COPIES - 1)]],
                         member_group[:hg * (COPIES - 1)], 64, 30)
    host_s = time.perf_counter() - t0
    got = b"".join(cons[int(cons_off[g]):int(cons_off[g]) + int(h_lens[g])].cpu().numpy().tobytes() for g in range(hg))
    same = got == want.cons.tobytes() and np.array_equal(want.distance, status[:hg * (COPIES - 1), 1])
    med = statistics.median(ms[64])
    say("round_host (numpy, one core) over %d of the groups at band 64: %.1f s = %.2f groups/s; the library: %.0f groups/s (x %.0f); same bytes and distances: %s" % (
        hg, host_s, hg / host_s, G / med * 1e3, (G / med * 1e3) / (hg / host_s), same))
al.close()
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
