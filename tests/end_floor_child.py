"""Batches and checks of tests/test_gpu_end_floor.py (TEST INFRASTRUCTURE), and its child process:
    python -m tests.end_floor_child
The library reads PC_JIT_MIN_CELLS once per process and PC_DISABLE_JIT at every launch, so one fresh process started with
PC_JIT_MIN_CELLS=1 and an empty user cache runs the end-rule scan over each kind of score kernel in turn: the generic one
(PC_DISABLE_JIT=1; pc_jit_stats stays 0, 0), the ones shipped in porechop_amd/kernel_cache (the panel's sequences: loaded,
none compiled) and run-time-compiled ones (sequences outside the panel)."""
import ctypes
import os
import random
import sys

import numpy as np
import torch

from tests import ref_pipeline
from tests.golden_io import load_panel
from tests.pairgen import mutate

FLAGSHIP = ("SQK-NSK007", "1D^2 part 2")
SOLO = "GGTCATTACGCAGTTCAGGACTTACA"                                     # a set with a start sequence only: a job that runs alone
PAIR24 = ("TTGACCGATACGGTCAAGCTTCAT", "CCATGAGTTCGATCCAGTAAGGCT")       # a 24-mer pair
LENS = (400, 150, 0, 3, 40, 149, 151)                                   # windows cut from, equal to and shorter than the read
COUNTS = (1, 63, 64, 65, 129, 1000)


def sets(flagship=True, extra=True):
    from porechop_amd.pipeline import AdapterSet
    out = []
    if flagship:
        out += [AdapterSet(a["name"], tuple(a["start"]), tuple(a["end"])) for a in load_panel() if a["name"] in FLAGSHIP]
        assert len(out) == 2
    if extra:
        out += [AdapterSet("solo", ("solo_start", SOLO), None),
                AdapterSet("pair24", ("pair24_start", PAIR24[0]), ("pair24_end", PAIR24[1]))]
    return out


def bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def paste(body, pos, piece):
    """piece over body[pos:], clipped to the body (its length stays)"""
    if pos < 0:
        piece, pos = piece[-pos:], 0
    return (body[:pos] + piece + body[pos + len(piece):])[:len(body)]


def make_reads(seed, count, adapter_sets):
    """count reads whose lengths run through LENS (the first one is 400 bases); most of those that can hold an adapter carry a
    copy at 70-100 % identity somewhere in their start window, half of them one in their end window: at the outer edge, a few
    bases in, flush with the window's inner edge, in the middle."""
    rng = random.Random(seed)
    starts = [s.start[1] for s in adapter_sets if s.start]
    ends = [s.end[1] for s in adapter_sets if s.end]
    out = []
    for i in range(count):
        ln = LENS[i % len(LENS)]
        body = bases(rng, ln)
        win = min(ln, 150)
        if ln >= 40:
            if rng.random() < 0.7:
                ad = mutate(rng, rng.choice(starts), rng.choice([0.0, 0.05, 0.15, 0.3]))
                body = paste(body, rng.choice([0, 0, 1, 6, 25, win - len(ad), win - len(ad) // 2, -5]), ad)
            if rng.random() < 0.5:
                ad = mutate(rng, rng.choice(ends), rng.choice([0.0, 0.05, 0.15, 0.3]))
                body = paste(body, ln - rng.choice([len(ad), len(ad), len(ad) + 1, len(ad) + 7, win, win - 3, len(ad) - 6]), ad)
        out.append(body)
    return out


def trims_of_records(rec, sides, p):
    """[J, R, 8] traced records -> the trim each pair would contribute by itself (0: none), as Pipeline.phase_b's torch path"""
    from porechop_amd.pipeline import _identities
    _, partial = _identities(rec)
    ok = rec[..., 0] != -1
    rs = rec[..., 0].to(torch.int64)
    re = rec[..., 1].to(torch.int64) + 1
    is_end = torch.tensor([bool(s) for s in sides], dtype=torch.bool, device=rec.device)[:, None]
    good = ok & (partial > p.end_threshold) & ((re - rs) >= p.min_trim_size)
    zero = torch.zeros_like(re)
    val_s = torch.where(good & (re != p.end_size), re + p.extra_end_trim, zero)
    val_e = torch.where(good & (rs != 0), p.end_size - rs + p.extra_end_trim, zero)
    return torch.clamp(torch.where(is_end, val_e, val_s), min=0)


class no_end_floor:
    """PC_NO_END_FLOOR=1 for the calls inside (the pipeline and the library read it at every call)"""

    def __enter__(self):
        os.environ["PC_NO_END_FLOOR"] = "1"

    def __exit__(self, *a):
        del os.environ["PC_NO_END_FLOOR"]


def check_batch(pl, raw, oracle=None, want=None):
    """Phase B of pl over the reads `raw`, all sets matching: the trims with the rule, without it and by the reference's
    sequential logic on the oracle (`want`: those, computed before) agree; record by record, a pair the rule skipped has no
    trim of its own in the unruled traced scan and every other record is identical.
    -> (pairs, pairs skipped, want, ruled records [J, R, 8], unruled records)"""
    from porechop_amd.batch import MODE_AUTO, MODE_TRACE
    from porechop_amd.synth import reads_from_strings
    assert "PC_NO_END_FLOOR" not in os.environ and pl.can_rule_phase_b
    p = pl.p
    reads, norm = reads_from_strings(raw)
    matching = list(range(len(pl.sets)))
    before = pl.stats.get("pairs_end_skipped_by_rule", 0)
    st1, et1 = pl.phase_b(reads, matching, end_rule=True)          # (batches this small take the traced-in-full route by default)
    pl.aligner.sync()
    skipped = pl.stats.get("pairs_end_skipped_by_rule", 0) - before
    with no_end_floor():
        assert not pl.can_rule_phase_b
        st0, et0 = pl.phase_b(reads, matching, end_rule=True)
        pl.aligner.sync()
    from porechop_amd.pipeline import END_RULE_MIN_READS
    assert len(raw) < END_RULE_MIN_READS
    st2, et2 = pl.phase_b(reads, matching)
    pl.aligner.sync()
    assert pl.stats.get("pairs_end_skipped_by_rule", 0) - before == skipped          # nothing skipped without the rule
    assert torch.equal(st0, st1) and torch.equal(et0, et1) and torch.equal(st2, st1) and torch.equal(et2, et1)
    if want is None:
        want = [ref_pipeline.phase_b(oracle.adapter_alignment, seq, pl.sets, matching, p) for seq in norm]
    got = list(zip(st1.cpu().tolist(), et1.cpu().tolist()))
    assert got == [tuple(w) for w in want], [(r, g, w) for r, (g, w) in enumerate(zip(got, want)) if g != tuple(w)][:5]
    # record by record
    jobs, where = pl._phase_b_jobs(reads, matching)
    sides = [w[0] for w in where]
    alone = [tuple(j[:3]) + (("alone", k),) for k, j in enumerate(jobs)]
    ruled = torch.stack(pl._scan_jobs(reads.arena, alone, MODE_AUTO, p.end_size, end_sides=sides))
    by_library = pl.aligner.floor_skipped()[0]
    pl._floor_seen += by_library                                  # (as phase_b notes them: not the middle scan's)
    full = torch.stack(pl._scan_jobs(reads.arena, jobs, MODE_TRACE, p.end_size))
    pl.aligner.sync()
    sentinel = torch.tensor([-1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=ruled.device)
    gone = (ruled == sentinel).all(dim=-1)
    failed = full[..., 0] == -1                                   # (an empty window: "no alignment" with or without the rule)
    assert torch.equal(ruled[~gone], full[~gone]), "a traced pair's record differs from the unruled scan's"
    assert int(trims_of_records(full, sides, p)[gone].max().item() if bool(gone.any()) else 0) == 0, "a skipped pair trims"
    assert int((gone & ~failed).sum()) <= by_library <= int(gone.sum()), (by_library, int(gone.sum()), int(failed.sum()))
    assert by_library == skipped
    pairs = int(gone.numel())
    assert pairs == len(jobs) * len(raw)
    return pairs, skipped, want, ruled, full


def jit_stats(al):
    c, d = ctypes.c_int64(0), ctypes.c_int64(0)
    al.lib.pc_jit_stats(ctypes.byref(c), ctypes.byref(d))
    return c.value, d.value


def main():
    from oracle.oracle import Oracle
    from porechop_amd.pipeline import Pipeline, ScanParams
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1" and "PC_NO_END_FLOOR" not in os.environ
    o = Oracle()
    # generic: no specialised kernel may run
    os.environ["PC_DISABLE_JIT"] = "1"
    pl = Pipeline(sets(), ScanParams())
    raw = make_reads(41, 129, pl.sets)
    pairs, skipped, want, _, _ = check_batch(pl, raw, o)
    assert 0 < skipped < pairs and jit_stats(pl.aligner) == (0, 0), (skipped, pairs, jit_stats(pl.aligner))
    pl.close()
    print("END_FLOOR_GENERIC_OK")
    del os.environ["PC_DISABLE_JIT"]
    # cached: the panel's sequences, every job alone -- their kernels ship with the library
    pl = Pipeline(sets(extra=False), ScanParams())
    raw4 = make_reads(42, 129, pl.sets)
    pairs, skipped, _, _, _ = check_batch(pl, raw4, o)
    st = jit_stats(pl.aligner)
    assert 0 < skipped < pairs and st[0] == 0 and st[1] >= 4, (skipped, pairs, st)
    pl.close()
    print("END_FLOOR_CACHED_OK")
    # compiled at run time: sequences outside the panel (the batch of the generic run: the same trims)
    pl = Pipeline(sets(), ScanParams())
    pairs, skipped2, _, _, _ = check_batch(pl, raw, want=want)
    st2 = jit_stats(pl.aligner)
    assert 0 < skipped2 < pairs and st2[0] >= 3, (skipped2, pairs, st2)
    pl.close()
    print("END_FLOOR_COMPILED_OK")


if __name__ == "__main__":
    sys.exit(main())
