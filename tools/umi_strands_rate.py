#!/usr/bin/env python3
"""Rate probe (GPU box) of the both-strands kernels (DESIGN.md sections 17 and 18), in the style of umi_neighbours_rate.py and
consensus_rate.py: one process, device events around the library call itself, the variants ALTERNATING, medians of `repeats`
repetitions with every repetition shown.  A record, not a gate.

   python tools/umi_strands_rate.py neighbours [n_keys] [repeats] [out.txt]
       n keys (5 % of them copies of other keys at 1 .. 3 edits, half of the copies mirrored) of 22 and of 44 bases at max_dist 2,
       in umi_groups.kernel_order: pc_umi_neighbours and pc_umi_neighbours_stranded on the same keys, in turn.
   python tools/umi_strands_rate.py pileup [groups] [repeats] [out.txt]
       consensus_rate.py's band-64 case (groups x 8 members, copies of 8 192-base originals at 6 % errors): the round with
       d_member_strand NULL, all 0, and half 1 (those members lie reverse-complemented in the arena: the same alignments), in
       turn.  Run from a tree whose library has no pc_consensus_round_stranded (the parent commit, for the comparison beside
       it) it measures pc_consensus_round alone.
The lines are APPENDED to out.txt (default profiles/umi_strands_rate.txt)."""
import ctypes
import random
import statistics
import sys
sys.path.insert(0, ".")
import numpy as np
import torch
import porechop_amd
from porechop_amd import consensus as cs
from porechop_amd import umi_groups as ug

mode = sys.argv[1] if len(sys.argv) > 1 else "neighbours"
size = int(sys.argv[2]) if len(sys.argv) > 2 else (65536 if mode == "neighbours" else 4096)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else "profiles/umi_strands_rate.txt"
dev = torch.device("cuda")
lines = []
_COMP = str.maketrans("ACGT", "TGCA")


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rc = call()
    e1.record()
    assert rc == 0, rc
    al.sync()
    return e0.elapsed_time(e1)


def report(name, v, extra=""):
    say("%s: median %.3f ms  (%s; spread %.3f)%s" % (name, statistics.median(v), " ".join("%.3f" % x for x in v), max(v) - min(v), extra))


al = porechop_amd.Aligner(["ACGTACGTACGT"])
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

if mode == "neighbours":
    n, MAX_DIST, CAP = size, 2, 1 << 22

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
            k = "".join(k)
            keys.append(k.translate(_COMP)[::-1] if len(keys) % 2 else k)
        rng.shuffle(keys)
        return keys

    pairs = torch.empty((CAP, 4), dtype=torch.int32, device=dev)
    found = torch.zeros(1, dtype=torch.int64, device=dev)
    sets = {}
    for length in (22, 44):
        planes, lens = ug.pack(make_keys(length, length))
        order = ug.kernel_order(planes, lens)
        sets[length] = (torch.from_numpy(np.ascontiguousarray(planes[order]).view(np.int64)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(lens[order])).to(dev), int(lens.max()))
    configs = [(22, False), (22, True), (44, False), (44, True)]
    ms, count = {c: [] for c in configs}, {}
    for rep in range(reps + 1):                         # (the first round is a warm-up: dropped)
        for length, stranded in configs:
            p, ln, max_len = sets[length]
            entry = al.lib.pc_umi_neighbours_stranded if stranded else al.lib.pc_umi_neighbours
            t = timed(lambda: entry(al._ctx, p.data_ptr(), ln.data_ptr(), n, max_len, MAX_DIST, pairs.data_ptr(), CAP, found.data_ptr(), stream))
            assert count.setdefault((length, stranded), int(found.item())) == int(found.item())
            if rep:
                ms[(length, stranded)].append(t)
    say("device: %s   keys: %d (5 %% copies at 1..3 edits, half of them mirrored)   max_dist: %d   kernel_order   repeats: %d (alternating)"
        % (torch.cuda.get_device_name(0), n, MAX_DIST, reps))
    for length in (22, 44):
        for stranded in (False, True):
            report("length %d (%d-bit kernel), %s" % (length, 32 if sets[length][2] <= 32 else 64, "stranded  " if stranded else "unstranded"),
                   ms[(length, stranded)], "  found %d" % count[(length, stranded)])
        say("length %d: stranded / unstranded = %.2f" % (length, statistics.median(ms[(length, True)]) / statistics.median(ms[(length, False)])))
else:
    G, COPIES, LENGTH, RATE, BAND = size, 8, 8192, 0.02, 64
    rng = np.random.default_rng(1818)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)

    def copy_of(orig):
        r = rng.random(orig.size)
        bases = np.where(r < RATE, (orig + rng.integers(1, 4, orig.size)) % 4, orig)
        deleted = (r >= RATE) & (r < 2 * RATE)
        inserted = (r >= 2 * RATE) & (r < 3 * RATE)
        counts = np.where(deleted, 0, np.where(inserted, 2, 1))
        out = np.repeat(bases, counts)
        starts = np.cumsum(counts) - counts
        out[starts[inserted]] = rng.integers(0, 4, int(inserted.sum()))
        return out

    codes = []
    for g in range(G):
        orig = rng.integers(0, 4, LENGTH)
        codes += [copy_of(orig) for _ in range(COPIES)]
    lens = np.array([s.size for s in codes], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)
    tmpl_idx = np.arange(G) * COPIES
    member_idx = np.array([g * COPIES + k for g in range(G) for k in range(1, COPIES)], dtype=np.int64)
    half = (np.arange(member_idx.size) % 2).astype(np.uint8)
    flipped = set(member_idx[half == 1].tolist())
    arenas = {False: torch.from_numpy(np.concatenate([letters[s] for s in codes] + [np.zeros(64, dtype=np.uint8)])).to(dev)}
    tmpl_off, tmpl_len = off[tmpl_idx].copy(), lens[tmpl_idx].astype(np.int32)
    first = (np.arange(G + 1, dtype=np.int64) * (COPIES - 1)).copy()
    M = member_idx.size
    d_off, d_len, d_grp = (torch.from_numpy(x).to(dev) for x in (off[member_idx].copy(), lens[member_idx].astype(np.int32),
                                                                 np.repeat(np.arange(G, dtype=np.int32), COPIES - 1)))
    cons_off = np.concatenate([[0], np.cumsum(cs.cons_capacity(tmpl_len.astype(np.int64)))])
    cons = torch.empty(int(cons_off[-1]) + 16, dtype=torch.uint8, device=dev)
    d_lens = torch.zeros(G, dtype=torch.int32, device=dev)
    voters = torch.zeros(G, dtype=torch.int32, device=dev)
    out = torch.zeros((M, 2), dtype=torch.int32, device=dev)
    stranded_entry = getattr(al.lib, "pc_consensus_round_stranded", None)
    variants = ["NULL"]
    if stranded_entry is not None:
        variants += ["all 0", "half 1"]
        arenas[True] = torch.from_numpy(np.concatenate([letters[3 - s[::-1]] if k in flipped else letters[s] for k, s in enumerate(codes)] +
                                                       [np.zeros(64, dtype=np.uint8)])).to(dev)
        strands = {"all 0": torch.zeros(M, dtype=torch.uint8, device=dev), "half 1": torch.from_numpy(half).to(dev)}

    def run(variant):
        arena = arenas[variant == "half 1"]
        head = (al._ctx, arena.data_ptr(), arenas[False].data_ptr(), tmpl_off.ctypes.data, tmpl_len.ctypes.data, first.ctypes.data, G,
                d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr())
        tail = (M, BAND, 30, 65535, 1, cons.data_ptr(), d_lens.data_ptr(), voters.data_ptr(), out.data_ptr(), None, None, stream)
        if variant == "NULL":
            return timed(lambda: al.lib.pc_consensus_round(*head, *tail))
        return timed(lambda: stranded_entry(*head, strands[variant].data_ptr(), *tail))

    ms, result = {v: [] for v in variants}, {}
    for rep in range(reps + 1):                         # (the first round is a warm-up: the scratch is allocated there)
        for v in variants:
            t = run(v)
            got = (out.cpu().numpy().tobytes(), d_lens.cpu().numpy().tobytes(), cons.cpu().numpy()[:64].tobytes())
            assert result.setdefault("all", got) == got, "the variants disagree"
            if rep:
                ms[v].append(t)
    say("device: %s   %d groups x %d members of %d bases at %.0f %% errors, band %d   %s   repeats: %d (alternating)" % (
        torch.cuda.get_device_name(0), G, COPIES, LENGTH, 300 * RATE, BAND,
        "this library has pc_consensus_round_stranded" if stranded_entry is not None else "a library without pc_consensus_round_stranded", reps))
    for v in variants:
        report("strand %-6s" % v, ms[v])
al.close()
with open(out_path, "a") as fh:
    fh.write("\n".join(lines) + "\n")
