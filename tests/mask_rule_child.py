"""The GPU checks of tests/test_gpu_mask_rule.py, run as a child process (TEST INFRASTRUCTURE):
    python -m tests.mask_rule_child
started with PC_JIT_MIN_CELLS=1 and a kernel cache of its own so that the specialised score kernels and their row-skipping
variants run from the first launch.
  1. pc_round_select against the header's host function (pc_mask_rule_must_realign) on random and edge records.
  2. Pipeline.phase_c with the mask rule against PC_NO_MASK_RULE=1 and against the reference's sequential logic on the oracle,
     at thresholds 75 and 90, on the floored route and under PC_NO_PASS2_FLOOR=1.
  3. The row-skip debug counters: round 0 counts skipping blocks, the mask rounds' launches -- which the fill rule chunks --
     count none, and the same scan call without the option counts them again.
  4. A batch most of whose reads are dirty, large enough that round 1 fills the device: the skip stays on there."""
import os
import random
import sys

import numpy as np
import torch

import porechop_amd
from oracle.oracle import Oracle
from porechop_amd.batch import mask_rule_must_realign
from tests import maskgen, ref_pipeline
from tests.golden_io import load_panel


# ---- 1. the selection kernel ---------------------------------------------------------------------------------------------
def select_case(al, rng, nact, S, floored):
    A = 2 * S if S > 1 else 3
    Dn = nact + 5
    set_of = np.array([min(a // 2, S - 1) for a in range(A)], dtype=np.int32)
    act = np.array(rng.sample(range(Dn), nact), dtype=np.int64)
    anyh = np.array([rng.random() < 0.8 for _ in range(nact)], dtype=np.uint8)
    a_hit = np.array([rng.randrange(A) for _ in range(nact)], dtype=np.int32)
    rec = np.zeros((A, Dn, 8), dtype=np.int32)
    rec[:, :, 2:] = 7
    for k in range(nact):
        d, h = int(act[k]), int(a_hit[k])
        hs = rng.randrange(0, 900)
        he = hs + rng.choice((-1, 0, 1, 20, 33))                 # inclusive end; -1: a hit interval of length 0
        for a in range(A):
            kind = rng.randrange(8)
            if kind == 0:
                r0, r1 = -1, 0
            elif kind == 1:                                      # meets the mask's left edge by 0 or 1 columns
                r1 = hs - rng.choice((0, 1)); r0 = r1 - rng.randrange(0, 30)
            elif kind == 2:                                      # ... its right edge
                r0 = he + 1 - rng.choice((0, 1)); r1 = r0 + rng.randrange(0, 30)
            elif kind == 3:
                r0 = rng.randrange(0, 1000); r1 = r0 - rng.randrange(1, 5)       # an odd record
            else:
                r0 = rng.randrange(0, 1000); r1 = r0 + rng.randrange(0, 40)
            rec[a, d, 0], rec[a, d, 1] = r0, r1
        rec[h, d, 0], rec[h, d, 1] = hs, he
    dev = "cuda"
    t = lambda x: torch.from_numpy(x).to(dev)
    rec_t, act_t, anyh_t, a_hit_t, set_t = t(rec), t(act), t(anyh), t(a_hit), t(set_of)
    need = torch.full((S, nact), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((S,), 9, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    rc = al.lib.pc_round_select(al._ctx, rec_t.data_ptr(), act_t.data_ptr(), anyh_t.data_ptr(), a_hit_t.data_ptr(), set_t.data_ptr(), nact, A, Dn, S,
                                1 if floored else 0, need.data_ptr(), counts.data_ptr(), s)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want = np.zeros((S, nact), dtype=np.uint8)
    for k in range(nact):
        if not anyh[k]:
            continue
        d, h = int(act[k]), int(a_hit[k])
        rs, re = int(rec[h, d, 0]), int(rec[h, d, 1]) + 1
        for a in range(h, A):
            if mask_rule_must_realign(a, h, rec[a, d, 0], rec[a, d, 1], rs, re, floored):
                want[set_of[a], k] = 1
    got = need.cpu().numpy()
    assert (got == want).all(), ("pc_round_select", nact, S, floored, int((got != want).sum()))
    assert counts.cpu().tolist() == want.sum(axis=1).tolist(), ("pc_round_select counts", nact, S, floored)
    assert 0 < want.sum() < want.size or nact == 1
    return nact * A


def check_select(al):
    rng = random.Random(77)
    records = 0
    for floored in (False, True):
        for nact in (1, 255, 256, 257):
            records += select_case(al, rng, nact, 1, floored)
        for nact in (1, 257):
            records += select_case(al, rng, nact, 98, floored)
    assert records >= 4096
    print("MASK_RULE select: %d records" % records)


# ---- 2, 3. phase_c ---------------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps the aligner's scan_device: after every call, the row-skip counters of that call (reading them clears them)."""
    def __init__(self, al):
        self.al, self.inner, self.calls = al, al.scan_device, []
        al.scan_device = self

    def __call__(self, *a, **kw):
        self.inner(*a, **kw)
        self.calls.append((self.al.row_skip_blocks(), a, kw))

    def close(self):
        self.al.scan_device = self.inner


def hits_of(h):
    return [getattr(h, f).cpu() for f in ("read", "adapter", "start", "end", "identity")] + [h.rounds, h.alignments]


def same(h0, h1, what):
    for x, y in zip(hits_of(h0), hits_of(h1)):
        assert (torch.equal(x, y) if torch.is_tensor(x) else x == y), what


def make_pipeline(threshold):
    from porechop_amd.pipeline import AdapterSet, Pipeline, ScanParams
    sets = [AdapterSet(a["name"], tuple(a["start"]) if a["start"] else None, tuple(a["end"]) if a["end"] else None) for a in load_panel()]
    p = ScanParams(middle_threshold=threshold)
    pl = Pipeline(sets, p)
    return pl, [i for i, s in enumerate(pl.sets) if s.name in maskgen.SETS3]


def check_phase_c(oracle, raw, threshold, n_touching, counters):
    from porechop_amd.synth import reads_from_strings
    pl, matching = make_pipeline(threshold)
    dreads, norm = reads_from_strings(raw)
    zero = torch.zeros(len(raw), dtype=torch.int32, device="cuda")
    pl.aligner.set_row_skip_debug(True)
    rec = Recorder(pl.aligner)
    results = {}
    for floor_off in (False, True):
        for rule_off in (False, True):
            for k, off in (("PC_NO_PASS2_FLOOR", floor_off), ("PC_NO_MASK_RULE", rule_off)):
                if off:
                    os.environ[k] = "1"
                else:
                    os.environ.pop(k, None)
            del rec.calls[:]
            kept0 = pl.stats.get("pairs_middle_kept_by_mask_rule", 0)
            h = pl.phase_c(dreads, zero, zero, matching)
            pl.aligner.sync()
            results[(floor_off, rule_off)] = (h, list(rec.calls), pl.stats.get("pairs_middle_kept_by_mask_rule", 0) - kept0)
    os.environ.pop("PC_NO_PASS2_FLOOR", None); os.environ.pop("PC_NO_MASK_RULE", None)
    base = results[(False, False)][0]
    assert base.rounds >= 3 and base.read.numel() >= len(raw) // 3
    for key, (h, calls, kept) in results.items():
        same(base, h, key)
        assert (kept > 0) == (not key[1]), (key, kept)
    # the rule launches fewer windows per mask round: the calls' window counts
    windows = lambda calls: sum(int(a[1].shape[0]) for _, a, _ in calls[1:])
    assert windows(results[(False, False)][1]) < windows(results[(False, True)][1])
    # the row-skip counters, floored route: round 0 skips rows, the mask rounds' chunked launches do not -- with the rule or without
    # (at the floors of 90 %, which the row skip is made for)
    for rule_off in ((False, True) if counters else ()):
        calls = results[(False, rule_off)][1]
        assert len(calls) >= 3 and calls[0][0][0] > 0, calls[0][0]
        assert all(blocks == (0, 0) for blocks, _, _ in calls[1:]), [c[0] for c in calls]
        assert all(kw.get("no_skip_underfilled") for _, _, kw in calls[1:]) and not calls[0][2].get("no_skip_underfilled")
    # ... and the same scan call without the option still counts them
    if counters:
        _, a, kw = results[(False, False)][1][1]
        assert kw.get("no_skip_underfilled")
        rec.inner(*a, **dict(kw, no_skip_underfilled=False))
        assert pl.aligner.row_skip_blocks()[0] > 0
    rec.close()
    # the reference's sequential logic on the reads with hits; the last n_touching reads are maskgen.touching_reads, in most of
    # which the mask of the 28-mer's hit takes exactly one column of the barcode's record
    got = {}
    for r, a, s, e, idn in zip(*(x.tolist() for x in hits_of(base)[:5])):
        got.setdefault(r, []).append((a, s, e, round(idn, 6)))
    changed = 0
    for r in sorted(got):
        want = [(a, s, e, round(f, 6)) for a, s, e, f in ref_pipeline.phase_c(oracle.adapter_alignment, norm[r], 0, 0, pl.middle_adapters, pl.p)]
        assert got[r] == want, (r, got[r], want)
        if r >= len(raw) - n_touching:
            assert len(want) == 2 and want[0][0] == 0 and want[1][0] in (4, 5), want
            changed += want[1][3] < 100.0
    assert changed >= n_touching // 2, changed
    pl.close()
    print("MASK_RULE phase_c threshold %g: %d hits, %d rounds" % (threshold, int(base.read.numel()), base.rounds))


# ---- 4. a mask round that fills the device keeps the skip -------------------------------------------------------------------
def check_big_round():
    from porechop_amd.synth import reads_from_strings
    n, ln = 160_000, 320
    rng = np.random.default_rng(3)
    body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, ln))]
    top = np.frombuffer(maskgen.Y_TOP.encode(), dtype=np.uint8)
    at = rng.integers(20, ln - 60, size=n)
    dirty = np.arange(n) % 16 != 0                                 # 15 of 16 reads hold the 28-mer
    for i in np.nonzero(dirty)[0]:
        body[i, at[i]:at[i] + top.size] = top
    raw = [row.tobytes().decode() for row in body]
    pl, matching = make_pipeline(90.0)
    dreads, _ = reads_from_strings(raw)
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    pl.aligner.set_row_skip_debug(True)
    rec = Recorder(pl.aligner)
    h = pl.phase_c(dreads, zero, zero, matching)
    pl.aligner.sync()
    rec.close()
    assert int(h.read.numel()) >= int(dirty.sum()) and h.rounds >= 1
    calls = rec.calls
    # round 1: 150 000 windows of one set, 2 344 tiles of 64 -- more than half of the 4 096 resident waves: one chunk, the skip on
    assert int(calls[1][1][1].shape[0]) >= 140_000 and calls[1][2].get("no_skip_underfilled")
    assert calls[0][0][0] > 0 and calls[1][0][0] > 0, [c[0] for c in calls]
    pl.close()
    print("MASK_RULE big round: blocks %d" % calls[1][0][0])


def main():
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1" and "PC_DISABLE_JIT" not in os.environ and "PC_NO_ROW_SKIP" not in os.environ
    oracle = Oracle()
    al = porechop_amd.Aligner([maskgen.Y_TOP, maskgen.Y_BOTTOM])
    check_select(al)
    al.close()
    raw = maskgen.reads(41, 2000, 1000, 2000) + maskgen.touching_reads(43, 48)
    check_phase_c(oracle, raw, 75.0, 48, False)
    check_phase_c(oracle, raw, 90.0, 48, True)
    check_big_round()
    print("MASK_RULE_CHILD_OK")


if __name__ == "__main__":
    sys.exit(main())
