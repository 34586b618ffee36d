#!/usr/bin/env python3
"""Cost probe (GPU box) of the consensus quality values (consensus_call_kernel<true> of pc_consensus.hip):
tools/consensus_rate.py's band-64 case -- `groups` groups of 8 members, copies of an 8 192-base original at 6 % errors, round 1 --
with and without a quality table, alternating in one process, medians of `repeats` with their spread, device events around the
call itself (pc_consensus_round_quality with the table, pc_consensus_round without).  The qualities of the first `host_groups`
groups are compared with consensus.round_host.
With the path of a library built from the PARENT commit's tree, that library's pc_consensus_round runs in the same alternation
(a context of its own in the same process): the call without a table launches the kernels the parent launches, so its median
must lie inside the spread of the parent's own repetitions.  A record, not a gate.
   python tools/consensus_quality_rate.py [groups] [repeats] [host_groups] [out.txt] [parent libporechop_amd.so]
                                                                  (default 4 096, 5, 4, profiles/consensus_quality_rate.txt, none)"""
import ctypes
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
host_g = int(sys.argv[3]) if len(sys.argv) > 3 else 4
out_path = sys.argv[4] if len(sys.argv) > 4 else "profiles/consensus_quality_rate.txt"
parent_path = sys.argv[5] if len(sys.argv) > 5 else None
COPIES, LENGTH, RATE, BAND = 8, 8192, 0.02, 64
dev = torch.device("cuda")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def copy_of(rng, orig):                                    # (tools/consensus_rate.py's)
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
say("%d groups x %d members, copies of %d-base originals at %.0f %% errors, band %d: %.1f MB of reads, made in %.1f s" % (
    G, COPIES, LENGTH, 300 * RATE, BAND, arena_h.size / 1e6, time.time() - t0))

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
qual = torch.empty_like(cons)
d_lens = torch.zeros(G, dtype=torch.int32, device=dev)
voters = torch.zeros(G, dtype=torch.int32, device=dev)
out = torch.zeros((M, 2), dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
table = cs.quality_table()

parent = parent_ctx = None
if parent_path:
    parent = ctypes.CDLL(parent_path)
    parent.pc_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    parent.pc_consensus_round.argtypes = al.lib.pc_consensus_round.argtypes
    parent.pc_consensus_round.restype = ctypes.c_int
    parent.pc_destroy.argtypes = [ctypes.c_void_p]
    parent_ctx = ctypes.c_void_p()
    assert parent.pc_create(ctypes.byref(parent_ctx), 0) == 0
    assert not hasattr(parent, "pc_consensus_round_quality"), "that library is not the parent's"


def run(which):
    head = (arena.data_ptr(), arena.data_ptr(), tmpl_off.ctypes.data, tmpl_len.ctypes.data, first.ctypes.data, G, d_off.data_ptr(),
            d_len.data_ptr(), d_grp.data_ptr())
    tail = (M, BAND, 30, 65535, 1, cons.data_ptr(), d_lens.data_ptr(), voters.data_ptr(), out.data_ptr(), None, None, ctypes.c_void_p(stream))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    if which == "table":
        rc = al.lib.pc_consensus_round_quality(al._ctx, *head, None, *tail, table.ctypes.data, qual.data_ptr())
    elif which == "plain":
        rc = al.lib.pc_consensus_round(al._ctx, *head, *tail)
    else:
        rc = parent.pc_consensus_round(parent_ctx, *head, *tail)
    assert rc == 0, rc
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


kinds = ["table", "plain"] + (["parent"] if parent else [])
for k in kinds:                                            # warm-up: the scratch is allocated here
    run(k)
ms = {k: [] for k in kinds}
for _ in range(reps):
    for k in kinds:
        ms[k].append(run(k))
al.sync()
names = dict(table="with a quality table (pc_consensus_round_quality)", plain="without a table (pc_consensus_round)",
             parent="the parent commit's library (pc_consensus_round)")
for k in kinds:
    say("%-52s %8.2f ms median of %d (min %.2f, max %.2f)   %.0f groups/s" % (
        names[k] + ":", statistics.median(ms[k]), reps, min(ms[k]), max(ms[k]), G / statistics.median(ms[k]) * 1e3))
med = {k: statistics.median(ms[k]) for k in kinds}
say("the table costs %+.2f ms a call (%+.2f %%)" % (med["table"] - med["plain"], 100 * (med["table"] - med["plain"]) / med["plain"]))
if parent:
    inside = min(ms["parent"]) <= med["plain"] <= max(ms["parent"])
    say("without a table against the parent: %+.2f ms; the median lies %s the parent's own spread %.2f .. %.2f ms" % (
        med["plain"] - med["parent"], "inside" if inside else "OUTSIDE", min(ms["parent"]), max(ms["parent"])))
    parent.pc_destroy(parent_ctx)

if host_g:
    hg = min(host_g, G)
    run("table")
    h_lens = d_lens.cpu().numpy()
    want = cs.round_host([seqs[g * COPIES].tobytes() for g in range(hg)], [seqs[m].tobytes() for m in member_idx[:hg * (COPIES - 1)]],
                         member_group[:hg * (COPIES - 1)], BAND, 30, qual_table=table)
    got_c = b"".join(cons[int(cons_off[g]):int(cons_off[g]) + int(h_lens[g])].cpu().numpy().tobytes() for g in range(hg))
    got_q = b"".join(qual[int(cons_off[g]):int(cons_off[g]) + int(h_lens[g])].cpu().numpy().tobytes() for g in range(hg))
    say("round_host over %d of the groups: same bytes %s, same qualities %s; their qualities: %s" % (
        hg, got_c == want.cons.tobytes(), got_q == want.qual.tobytes(),
        ", ".join("Q%d x %d" % (q, n) for q, n in zip(*np.unique(want.qual, return_counts=True)))))
al.close()
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
