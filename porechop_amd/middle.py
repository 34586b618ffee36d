"""The middle scan's host side: the per-read glue steps as one contract, and the mask-and-realign loop of
Pipeline.phase_c written once against it.

The contract is that of the Aligner's single-launch kernels (pc_middle.hip: trim_windows, middle_hits, round_consume,
round_consume_select, group_survivors, and copy_windows).  TorchGlue is the same contract in torch expressions, for aligners
without the kernels (the oracle stand-ins of the tests) and for PC_NO_FUSED_GLUE=1; choose_glue picks one per call.
MiddleScan is one phase_c call: Pipeline.phase_c, middle_hit_paths and middle_adapter_list stay the ways in."""
from collections import namedtuple
from dataclasses import dataclass, field

import os

import torch

from .batch import MODE_SCORE, MODE_TWO_PASS, RESULT_INTS, mask_rule_gate


def switch_on(name):
    """True when the PC_NO_* switch `name` is set to anything but "" or "0".  Read at call time: tests flip the switches
    between calls in one process."""
    return os.environ.get(name, "0") not in ("", "0")


def add_stat(stats, key, value):
    stats[key] = stats.get(key, 0) + value


def set_positions(mask, count):
    """The positions at which `mask` is set, ascending, when their number is already on the host (no further round trip
    where torch has nonzero_static)."""
    if hasattr(torch, "nonzero_static"):
        return torch.nonzero_static(mask, size=count).flatten()
    return torch.nonzero(mask).flatten()


def must_realign_torch(a, cur, read_start, read_end, rs, re, floored_positive):
    """pcm::must_realign (csrc/pc_mask_rule.h) over tensors that broadcast against one another, for aligners without the native
    selection step; tests/test_mask_rule_pipeline_cpu.py holds it against the header's function record by record."""
    changed = torch.where(read_start == -1, torch.full_like(read_start, 0 if floored_positive else 1, dtype=torch.bool),
                          (re > rs) & ((read_start < 0) | (read_end < read_start) | ((read_start < re) & (read_end >= rs))))
    return (changed & (a > cur)) | (a == cur)


def _round6(x):
    """float("%f" % x) for non-negative doubles: the value Python parses back from the C side's six printed decimals.
    The quotient is a TRUE division by a one-element device tensor: `tensor / 1e6` with a Python scalar is evaluated by
    PyTorch as a multiplication by the rounded reciprocal, which lands one ulp off the correctly rounded value for about
    one identity in seven (seen as 33 of 238 presence-table entries differing from the host's in the last bit)."""
    million = torch.full((1,), 1e6, dtype=torch.float64, device=x.device)
    return torch.round(x * 1e6) / million


def _identities(rec):
    """float64 (full, partial) exactly as nanopore_read.py:476-491 parses them: the C side prints
    (100.0*matches)/len with %f and Python float()s it back; rounding the unrounded double to six decimals
    reproduces the printed digits as long as no value lies within 5e-7 of a rounding boundary without being on
    it -- identities are ratios of small integers (len <= a few hundred), whose six-decimal digits are never
    within 1e-8 of a tie."""
    m = rec[..., 5].to(torch.float64)
    partial = _round6(100.0 * m / rec[..., 6].to(torch.float64))
    full = _round6(100.0 * m / rec[..., 7].to(torch.float64))
    return full, partial


def trimmed_interval(length, start_trim, end_trim):
    """[s, e) of seq[start_trim : len(seq) - end_trim] with Python's slice semantics, the whole read
    when both trims are 0 (nanopore_read.py:56-62): a start beyond the end clamps, a negative end
    index counts from the end.  Tensors in, int64 tensors out (e < s means empty)."""
    ln = length.to(torch.int64)
    s_pos = torch.clamp(start_trim.to(torch.int64), max=ln)
    e_pos = ln - end_trim.to(torch.int64)
    e_pos = torch.where(e_pos < 0, torch.clamp(ln + e_pos, min=0), e_pos)
    untouched = (start_trim == 0) & (end_trim == 0)
    s_pos = torch.where(untouched, torch.zeros_like(s_pos), s_pos)
    e_pos = torch.where(untouched, ln, e_pos)
    return s_pos, e_pos


def middle_mask_tables(read, start, end):
    """What Aligner.middle_paths needs to see each middle hit's read masked as its round of mask-and-realign saw it, from the
    hit list alone (MiddleHits lists a read's hits in discovery order; masking never moves a coordinate).
    read int64 [H], start / end int32 [H] -> (intervals int32 [H, 2], mask_base int64 [H], mask_count int32 [H]):
    intervals are the hits' [start, end) stably sorted by read -- no interval is copied twice -- and hit h at rank k within
    its read gets mask_base = its read's first row and mask_count = k: the rows of its read's earlier hits."""
    H = int(read.shape[0])
    dev = read.device
    if H == 0:
        return (torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev))
    order = torch.sort(read, stable=True).indices
    sorted_read = read[order]
    row = torch.arange(H, dtype=torch.int64, device=dev)
    first = torch.ones(H, dtype=torch.bool, device=dev)
    first[1:] = sorted_read[1:] != sorted_read[:-1]
    first_row = torch.cummax(torch.where(first, row, torch.zeros_like(row)), 0).values
    intervals = torch.stack([start[order], end[order]], dim=1).to(torch.int32).contiguous()
    mask_base = torch.empty(H, dtype=torch.int64, device=dev)
    mask_base[order] = first_row
    mask_count = torch.empty(H, dtype=torch.int32, device=dev)
    mask_count[order] = (row - first_row).to(torch.int32)
    return intervals, mask_base, mask_count


class TorchGlue:
    """The Aligner's glue steps of the middle scan (batch.py, "the glue of the middle scan") in torch expressions: the same
    arguments, result tuples and statistic encodings, on whatever device the tensors are."""
    STAT_BIG = 1 << 40

    def trim_windows(self, off, length, start_trim, end_trim):
        """-> (toff int64[R], tlen int32[R], stats int64[4]: live, longest, STAT_BIG - shortest non-empty (0: none), sum)"""
        s_pos, e_pos = trimmed_interval(length, start_trim, end_trim)
        tlen = torch.clamp(e_pos - s_pos, min=0).to(torch.int32)
        toff = off + s_pos
        if not int(off.shape[0]):
            return toff, tlen, torch.zeros(4, dtype=torch.int64, device=off.device)
        pos_len = tlen > 0
        t64 = tlen.to(torch.int64)
        stats = torch.stack([pos_len.sum(), t64.max(), torch.where(pos_len, self.STAT_BIG - t64, torch.zeros_like(t64)).max(),
                             t64.sum()])
        return toff, tlen, stats

    def middle_hits(self, rec, threshold):
        """rec int32[..., 8] -> (full float64[...]: 0.0 for "no alignment" and for an all-zero "not computed" record, whose
        identity is 0 / 0; hit bool[...])"""
        full, _ = _identities(rec)
        aligned = rec[..., 0] != -1
        full = torch.nan_to_num(torch.where(aligned, full, torch.zeros_like(full)), nan=0.0)
        return full, (full >= threshold) & aligned

    def group_survivors(self, mask, gmask):
        """mask int32[n, words], gmask int32[G, words] -> (cand bool[G, n], counts int64[G])"""
        cand = ((mask[None, :, :] & gmask[:, None, :]) != 0).any(dim=2)
        return cand, cand.sum(dim=1)

    def round_consume(self, full_all, rec_all, cur, act, threshold):
        """One consuming step of mask-and-realign -> (anyh bool[n], a_hit int32[n], cnt int64[n], stats int64[4]: alignments
        consumed, reads that hit, STAT_BIG - the first adapter among them (0: none), bases to mask)"""
        return self.round_consume_select(full_all, rec_all, cur, act, threshold, None, 0, False)[:4]

    def round_consume_select(self, full_all, rec_all, cur, act, threshold, set_of, nsets, floored_positive):
        """round_consume and which adapter sets (set_of int32[A]) the next round must scan for which of the reads that hit
        (must_realign_torch) -> (anyh, a_hit, cnt, stats int64[4 + nsets]: the four statistics, then the reads that need
        each set; need bool[nsets, n])"""
        A, n, dev = int(full_all.shape[0]), int(act.shape[0]), act.device
        if not n:
            e = torch.zeros(0, dtype=torch.int64, device=dev)
            return e.to(torch.bool), e.to(torch.int32), e, torch.zeros(4 + nsets, dtype=torch.int64, device=dev), e.to(torch.bool).view(nsets, 0)
        arow = torch.arange(A, device=dev)[:, None]
        c = cur[act]
        hm = (full_all[:, act] >= threshold) & (rec_all[:, act, 0] != -1) & (arow >= c[None, :])
        anyh = hm.any(dim=0)
        a_hit = hm.to(torch.int32).argmax(dim=0)
        used = torch.where(anyh, a_hit - c + 1, A - c)
        r_all = rec_all[a_hit, act]
        cnt_all = torch.where(anyh, torch.clamp(r_all[:, 1] + 1 - r_all[:, 0], min=0), torch.zeros_like(r_all[:, 0])).to(torch.int64)
        stats = torch.stack([used.sum(), anyh.sum(), torch.where(anyh, self.STAT_BIG - a_hit, torch.zeros_like(a_hit)).max(),
                             cnt_all.sum()])
        need = None
        if nsets:
            must = must_realign_torch(arow, a_hit[None, :], rec_all[:, act, 0], rec_all[:, act, 1], r_all[:, 0][None, :],
                                      (r_all[:, 1] + 1)[None, :], floored_positive) & anyh[None, :]
            need = torch.zeros((nsets, n), dtype=torch.int32, device=dev).index_add_(0, set_of.to(torch.int64), must.to(torch.int32)) > 0
            stats = torch.cat([stats, need.sum(dim=1)])
        return anyh, a_hit.to(torch.int32), cnt_all, stats, need

    def copy_windows(self, arena, src_off, length, dst, dst_off, pad):
        """Window i of `arena` -> dst[dst_off[i]:], padded with `pad` up to dst_off[i + 1]"""
        n, dev = int(src_off.shape[0]), dst.device
        total = int(dst_off[-1])
        seg = torch.repeat_interleave(torch.arange(n, device=dev), dst_off[1:] - dst_off[:-1])
        pos = torch.arange(total, device=dev, dtype=torch.int64) - dst_off[:-1][seg]
        inside = pos < length[seg]
        src = src_off[seg] + torch.clamp(pos, max=(length.to(torch.int64) - 1)[seg])
        dst[:total] = torch.where(inside, arena[src], torch.full_like(src, pad, dtype=torch.uint8))


GLUE_STEPS = ("trim_windows", "middle_hits", "round_consume", "round_consume_select", "group_survivors")


def choose_glue(aligner):
    """The glue of one call: the aligner itself when it has the native steps and PC_NO_FUSED_GLUE is unset or 0 (read per
    call), else the torch glue -- whose copy_windows still goes to the aligner's kernel wherever there is one.  `glue is
    aligner` says which it is: the torch glue runs without score floors."""
    if all(hasattr(aligner, step) for step in GLUE_STEPS) and not switch_on("PC_NO_FUSED_GLUE"):
        return aligner
    glue = TorchGlue()
    if hasattr(aligner, "copy_windows"):
        glue.copy_windows = aligner.copy_windows
    return glue


@dataclass
class MiddleHits:
    read: torch.Tensor       # int64 [H]   read index
    adapter: torch.Tensor    # int32 [H]   index into Pipeline.middle_adapters
    start: torch.Tensor      # int32 [H]   read_start in trimmed-read coordinates
    end: torch.Tensor        # int32 [H]   read_end (exclusive)
    identity: torch.Tensor   # float64 [H] full-adapter identity
    rounds: int = 0
    alignments: int = 0

    @classmethod
    def none(cls, dev, rounds=0, alignments=0):
        return cls(*(torch.empty(0, dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.float64)),
                   rounds, alignments)


# The reads that are not empty after their trims: `live` indexes the call's reads, off / length are their windows.
Windows = namedtuple("Windows", "live off length max_len ragged typ_len")
# What round 0 leaves, by any route.  Dense: rec [A, L, 8], full / hit [A, L].  Sparse (a and w given): record k is that of
# adapter a[k] and window w[k], and every pair that is not listed is proven not to be a hit.
Records = namedtuple("Records", "rec full hit a w", defaults=(None, None))
# One consuming step: per active read anyh, a_hit, cnt (bases to mask) and, with the mask rule, need[set]; on the host the
# alignments consumed, the reads that hit, the first adapter among them (A: none), the bases to mask, the reads that need each set.
Consumed = namedtuple("Consumed", "anyh a_hit cnt need n_used n_hit a0 n_mask set_counts")


@dataclass
class Rounds:
    """What a round of mask-and-realign carries: the records [A, Dn, 8] and identities [A, Dn] of the dirty reads' current
    masked state, the adapter each stands at, the reads still active, their private copies, and the call's counters."""
    d_sel: torch.Tensor = None           # the dirty reads (indices into Windows.live), increasing
    rec_all: torch.Tensor = None
    full_all: torch.Tensor = None
    cur: torch.Tensor = None
    act: torch.Tensor = None
    dirty: torch.Tensor = None           # the copies, back to back: read d at dirty[d_off[d] : d_off[d] + dlen[d]]
    d_off: torch.Tensor = None
    dlen: torch.Tensor = None
    dmax: int = 0
    dtyp: int = 0
    n_align: int = 0                     # alignments the reference performs
    n_spec: int = 0                      # speculative ones, discarded
    n_kept: int = 0                      # of the rounds' (A - a0) x active pairs, those the mask rule kept
    scheduled: int = 0
    rounds: int = 0
    found: list = field(default_factory=list)      # per round: (read, adapter, start, end, identity) of its hits


class MiddleScan:
    """One Pipeline.phase_c call (its docstring says what is computed): round 0 by one of three routes, then the rounds."""

    def __init__(self, pl, reads, ads_sets, prove, prefilter):
        self.pl, self.p, self.dev, self.al = pl, pl.p, pl.device, pl.aligner
        self.glue = choose_glue(pl.aligner)
        self.reads, self.prove, self.prefilter = reads, prove, prefilter
        self.ads_sets = ads_sets
        self.A = len(ads_sets)
        self.aidx = [pl.seq_index[a[1]] for a, _ in ads_sets]
        self.hint = [("set", si) for _, si in ads_sets]
        self.thr = pl.p.middle_threshold
        self.floors = self.ks = None
        self.packed_only = False

    def run(self, start_trim, end_trim):
        win = self.windows(start_trim, end_trim)
        if win is None:
            return MiddleHits.none(self.dev)
        self.packed_only = self.reads.arena is None
        if self.packed_only and not self.prefilter:
            self.reads.materialize(self.al)                          # every pair runs the DP: every base is needed as a byte
            self.packed_only = False
        records = self.round0(win)
        st = self.dirty_reads(win, records)
        if st.act is not None:
            self.rounds(win, st)
        self.account(st)
        if not st.found:
            return MiddleHits.none(self.dev, st.rounds, st.n_align)
        return MiddleHits(*(torch.cat(col) for col in zip(*st.found)), st.rounds, st.n_align)

    def windows(self, start_trim, end_trim):
        """masked_seq = seq[start_trim : len - end_trim] with Python slice semantics (nanopore_read.py:56-62) -> the Windows
        that are not empty, or None when all are.
        (one round trip: how many reads are left after trimming, and the extremes / mean of their lengths)"""
        reads = self.reads
        toff, tlen, stats = self.glue.trim_windows(reads.off, reads.length, start_trim, end_trim)
        n_live, longest, shortest, total = (int(x) for x in stats.cpu())
        shortest = self.glue.STAT_BIG - shortest if shortest else 0
        if n_live == 0:
            return None
        if n_live == reads.n:
            live = torch.arange(reads.n, device=self.dev)
            loff, llen = toff, tlen
        else:
            live = set_positions(tlen > 0, n_live)
            loff, llen = toff[live], tlen[live]
        # (windows of different lengths are handed over longest first even when they differ by a per cent -- 8-kb reads that lost
        # 0..150 bases to their trims: tiles of nearly one length keep the specialised score kernel on its block-resolved path;
        # skipping the sort for such batches was measured: 0.3 ms of glue saved, 1.6 ms of scan lost at 1 M reads)
        return Windows(live, loff, llen, longest, longest != shortest, total // n_live)

    # ---- round 0: all adapters x all reads, unmasked --------------------------------------------------------------------
    def round0(self, win):
        if self.prefilter:
            return self.round0_prefiltered(win)
        bounds = [self.pl.identity_score_bound(len(self.pl.seqs[ai]), self.thr) for ai in self.aidx] if self.prove else None
        if self.prove and all(b is not None for b in bounds):
            return self.round0_proven(win, bounds)
        return self.round0_default(win)

    def jobs0(self, win):
        return [(ai, win.off, win.length, h) for ai, h in zip(self.aidx, self.hint)]

    def round0_default(self, win):
        """Every pair through the two-pass scan.  The identity bound of prove=True goes down as a score floor per job: the
        library decides between its two passes which pairs can still be hits and traces only those (pc_scan_device_floored);
        the others get the "no alignment" record, which is "not a hit".  PC_NO_PASS2_FLOOR=1: every pair traced."""
        pl = self.pl
        if not self.prove and self.glue is self.al and hasattr(self.al, "floor_skipped") and pl.packed_kernels() \
                and not switch_on("PC_NO_PASS2_FLOOR"):
            floors = [pl.identity_score_bound(len(pl.seqs[ai]), self.thr) for ai in self.aidx]
            self.floors = None if any(b is None for b in floors) else floors
        outs = pl._scan_jobs(self.reads.arena, self.jobs0(win), MODE_TWO_PASS, win.max_len, sort_lengths=win.ragged, typ_len=win.typ_len,
                             floors=self.floors)
        rec = torch.stack(outs)
        return Records(rec, *self.glue.middle_hits(rec, self.thr))                   # [A, L] each

    def round0_proven(self, win, bounds):
        """The score-only pass for every pair, the traceback for those whose score can still mean a hit; the others keep an
        all-zero record (rs = 0, lengths 0), which is "not a hit": its 0 / 0 identity counts as 0."""
        pl, A, arena = self.pl, self.A, self.reads.arena
        scan = dict(sort_lengths=win.ragged, typ_len=win.typ_len)
        score = torch.stack(pl._scan_jobs(arena, self.jobs0(win), MODE_SCORE, win.max_len, **scan))[:, :, 4]      # [A, L]
        cand = torch.nonzero(score >= pl._const(bounds)[:, None])                     # adapter-major
        counts = torch.bincount(cand[:, 0], minlength=A).cpu().numpy()
        recs = torch.zeros((A, int(win.live.numel()), RESULT_INTS), dtype=torch.int32, device=self.dev)
        cjobs, csel, pos = [], [], 0
        for a in range(A):
            if counts[a]:
                sel = cand[pos:pos + int(counts[a]), 1]
                pos += int(counts[a])
                cjobs.append((self.aidx[a], win.off[sel], win.length[sel])); csel.append((a, sel))     # (different windows per adapter: never fused)
        if cjobs:
            for (a, sel), o in zip(csel, pl._scan_jobs(arena, cjobs, MODE_TWO_PASS, win.max_len, **scan)):
                recs[a, sel] = o
        add_stat(pl.stats, "pairs_middle_traced_after_proof", int(counts.sum()))
        return Records(recs, *self.glue.middle_hits(recs, self.thr))

    def round0_prefiltered(self, win):
        """Only the pairs the exact prefilter cannot exclude (Pipeline._prefiltered_scan): sparse records."""
        pl = self.pl
        self.ks = [self.al.max_edits(len(pl.seqs[ai]), self.thr) for ai in self.aidx]
        sa, sw, sr = pl._prefiltered_scan(self.reads.arena, win.off, win.length, win.max_len, list(range(self.A)), self.aidx, self.hint, self.ks,
                                          win.ragged, win.typ_len, packed_reads=self.reads if self.packed_only else None)
        self.packed_only = self.packed_only and self.reads.arena is None      # (the packed route may have been refused: everything unpacked)
        return Records(sr, *self.glue.middle_hits(sr.contiguous(), self.thr), a=sa, w=sw)

    # ---- the dirty reads: those with a hit in round 0 --------------------------------------------------------------------
    def dirty_reads(self, win, records):
        """-> the Rounds' starting state; without a dirty read, its counters alone.
        (one round trip: the dirty reads -- those with a hit -- their number, longest, total padded size and mean length)"""
        A, L, llen = self.A, int(win.live.numel()), win.length
        if records.a is not None:
            dmask = torch.zeros(L, dtype=torch.int32, device=self.dev).index_add_(0, records.w, records.hit.to(torch.int32)) > 0
        else:
            dmask = records.hit.any(dim=0)
        dstride_all = (llen.to(torch.int64) + (8 + 15)) // 16 * 16
        zero64 = torch.zeros((), dtype=torch.int64, device=self.dev)
        mm2 = torch.stack([dmask.sum(), torch.where(dmask, llen.to(torch.int64), zero64).max(), torch.where(dmask, dstride_all, zero64).sum(),
                           torch.where(dmask, llen.to(torch.int64), zero64).sum()]).cpu()
        Dn = int(mm2[0])
        st = Rounds(n_align=A * (L - Dn), scheduled=A * Dn)          # (the dirty reads' alignments are counted as consumed)
        if Dn == 0:
            return st
        st.d_sel = set_positions(dmask, Dn)
        st.rec_all, st.full_all = self.dirty_table(records, st.d_sel, L, Dn)
        st.dmax, dtotal, st.dtyp = int(mm2[1]), int(mm2[2]), int(mm2[3]) // Dn
        self.private_copies(win, st, Dn, dtotal)
        st.cur = torch.zeros(Dn, dtype=torch.int64, device=self.dev)     # adapter each dirty read is at
        st.act = torch.arange(Dn, device=self.dev)
        return st

    def dirty_table(self, records, d_sel, L, Dn):
        """[A, Dn, 8] records and [A, Dn] identities of the dirty reads, for their current (unmasked) state."""
        A = self.A
        if records.a is None:
            return torch.stack([o[d_sel] for o in records.rec]), records.full[:, d_sel]
        # from the sparse records of the dirty reads (no boolean masks -- each is a nonzero, a host round trip: the records
        # of reads that are not dirty all go to one spare row behind the table)
        where = torch.full((L,), -1, dtype=torch.int64, device=self.dev)
        where[d_sel] = torch.arange(Dn, device=self.dev)
        w2 = where[records.w]
        flat = torch.where(w2 >= 0, records.a * Dn + w2, torch.full_like(w2, A * Dn))
        rec_flat = torch.zeros((A * Dn + 1, RESULT_INTS), dtype=torch.int32, device=self.dev)
        full_flat = torch.zeros(A * Dn + 1, dtype=torch.float64, device=self.dev)
        rec_flat[flat] = records.rec
        full_flat[flat] = records.full
        return rec_flat[:A * Dn].view(A, Dn, RESULT_INTS), full_flat[:A * Dn].view(A, Dn)

    def private_copies(self, win, st, Dn, dtotal):
        """Private, maskable copies of the dirty reads, back to back whatever their lengths (each padded with N to a multiple
        of 16 bytes plus slack: the kernels read whole dwords)."""
        st.dlen = win.length[st.d_sel].contiguous()
        dstride = (st.dlen.to(torch.int64) + (8 + 15)) // 16 * 16
        d_ends = torch.zeros(Dn + 1, dtype=torch.int64, device=self.dev)
        d_ends[1:] = torch.cumsum(dstride, 0)
        st.dirty = torch.empty(dtotal + 64, dtype=torch.uint8, device=self.dev)
        st.dirty[dtotal:] = ord("N")
        st.d_off = d_ends[:-1]
        src = win.off[st.d_sel].contiguous()
        if self.packed_only:                                         # (d_sel is ascending: torch.unique)
            self.al.unpack_windows(self.reads.plane, self.reads.exc, src, st.dlen, st.dirty, d_ends, ord("N"))
        else:
            self.glue.copy_windows(self.reads.arena, src, st.dlen, st.dirty, d_ends, ord("N"))

    # ---- the rounds ------------------------------------------------------------------------------------------------------
    def mask_rule(self):
        """The mask rule (csrc/pc_mask_rule.h): a mask only lowers substitution scores, so the record of a pair whose read
        interval the mask does not touch -- and, under positive floors, every "no alignment" record -- is provably the one
        already held.  A round then scans, per adapter SET (its sequences share one window list and fuse into the dual
        kernel), only the reads that have a record of the set the mask can have changed.  Behind the rule's gate (letters
        A/C/G/T/U, no wildcards, mismatch <= match); PC_NO_MASK_RULE=1, read per call: every round as before.  The proving
        routes keep their rounds (their tables hold all-zero "not computed" records, of which the rule says nothing).
        -> None, or (set_of int32[A] on the device: the dense set index of every middle adapter, the adapters of each set,
        floored_positive)"""
        pl = self.pl
        if self.prefilter or self.prove or switch_on("PC_NO_MASK_RULE") \
                or not mask_rule_gate([pl.seqs[ai] for ai in self.aidx], self.p.scores, self.p.wildcards):
            return None
        set_ids = sorted(set(si for _, si in self.ads_sets))
        set_of = [set_ids.index(si) for _, si in self.ads_sets]
        set_adapters = [[a for a in range(self.A) if set_of[a] == s] for s in range(len(set_ids))]
        return pl._const(set_of, dtype=torch.int32), set_adapters, self.floors is not None and all(f > 0 for f in self.floors)

    def rounds(self, win, st):
        rule = self.mask_rule()
        while True:
            c = self.consume(st, rule)
            st.n_align += c.n_used
            st.n_spec += st.scheduled - c.n_used
            if c.n_hit == 0:
                return
            hidx = self.mask_hits(win, st, c)
            st.rounds += 1
            st.scheduled = (self.A - c.a0) * int(st.act.numel())
            if rule is not None:
                self.realign_by_rule(win, st, c, hidx, rule[1])
            else:
                self.realign_from(win, st, c.a0)

    def consume(self, st, rule):
        """Per active read: adapters cur.. in order, up to and including the first hit.
        (one round trip per round: alignments consumed, reads that hit, the first adapter among them, bases to mask -- and,
        with the rule, how many of the reads that hit need each set: the same buffer)"""
        need = None
        if rule is not None:
            anyh, a_hit, cnt, stats, need = self.glue.round_consume_select(st.full_all, st.rec_all, st.cur, st.act, self.thr, rule[0],
                                                                           len(rule[1]), rule[2])
        else:
            anyh, a_hit, cnt, stats = self.glue.round_consume(st.full_all, st.rec_all, st.cur, st.act, self.thr)
        stats = [int(x) for x in stats.cpu()]
        a0 = self.glue.STAT_BIG - stats[2] if stats[2] else self.A
        return Consumed(anyh, a_hit, cnt, need, stats[0], stats[1], a0, stats[3], stats[4:])

    def mask_hits(self, win, st, c):
        """Keep the round's hits, mask them in the copies, and leave the reads that hit as the active ones, each standing at
        the adapter that hit (the reference re-aligns it) -> their positions among the reads that were active."""
        hidx = set_positions(c.anyh, c.n_hit)
        hsel = st.act[hidx]
        ah = c.a_hit[hidx].to(torch.int64)
        r = st.rec_all[ah, hsel]
        rs, re = r[:, 0], r[:, 1] + 1
        st.found.append((win.live[st.d_sel[hsel]], ah.to(torch.int32), rs, re, st.full_all[ah, hsel]))
        # masked_seq[rs:re] = '-' * n: the masked positions of all hits as one index list
        cnt = c.cnt[hidx]
        first = torch.cumsum(cnt, 0) - cnt
        run = torch.repeat_interleave(st.d_off[hsel] + rs.to(torch.int64) - first, cnt, output_size=c.n_mask)
        st.dirty.index_fill_(0, run + torch.arange(c.n_mask, device=self.dev, dtype=torch.int64), ord("-"))   # (x[idx] = scalar uploads the scalar: a round trip)
        st.cur[hsel] = ah
        st.act = hsel
        return hidx

    def realign_by_rule(self, win, st, c, hidx, set_adapters):
        """The next round's records under the mask rule: per set with a non-zero count, one job per sequence of the set over
        the reads that need the set.  The windows go longest first (one argsort a round, as _scan_jobs would per window
        list); one nonzero lists the (set, read) pairs set by set, and the host cuts that list at the counts it already holds."""
        pl, act = self.pl, st.act
        act_s, o_s, l_s, need_h = act, st.d_off[act], st.dlen[act], c.need[:, hidx]
        if win.ragged:
            perm = torch.argsort(l_s, descending=True, stable=True)
            act_s, o_s, l_s, need_h = act[perm], o_s[perm], l_s[perm], need_h[:, perm]
        which = set_positions(need_h.reshape(-1), sum(c.set_counts)) % c.n_hit
        o_f, l_f, act_f = o_s[which], l_s[which], act_s[which]
        rjobs, rmeta, at = [], [], 0
        for s, count in enumerate(c.set_counts):
            if count:
                o_c, l_c, a_c = o_f[at:at + count], l_f[at:at + count], act_f[at:at + count]
                at += count
                for a in set_adapters[s]:
                    if a >= c.a0:
                        rjobs.append((self.aidx[a], o_c, l_c, self.hint[a])); rmeta.append((a, a_c))
        st.n_kept += st.scheduled - sum(int(a_c.shape[0]) for _, a_c in rmeta)
        if not rjobs:
            return
        res, out_r, rec_off = pl._scan_jobs(st.dirty, rjobs, MODE_TWO_PASS, st.dmax, with_layout=True, presorted=win.ragged, typ_len=st.dtyp,
                                            floors=[self.floors[a] for a, _ in rmeta] if self.floors is not None else None,
                                            no_skip_underfilled=True)
        full_r = self.glue.middle_hits(out_r, self.thr)[0]
        for (a, a_c), r_, ro in zip(rmeta, res, rec_off):
            st.rec_all[a, a_c] = r_
            st.full_all[a, a_c] = full_r[ro:ro + int(a_c.shape[0])]

    def realign_from(self, win, st, a0):
        """The next round's records without the rule: every adapter from a0 on against every active read."""
        pl, A, act = self.pl, self.A, st.act
        o_act, l_act = st.d_off[act], st.dlen[act]
        if self.prefilter:                                           # the masked reads go through the same proof first
            rb, rw, rr = pl._prefiltered_scan(st.dirty, o_act, l_act, st.dmax, list(range(a0, A)), self.aidx, self.hint, self.ks, win.ragged, st.dtyp)
            outs_r = torch.zeros((A - a0, int(act.numel()), RESULT_INTS), dtype=torch.int32, device=self.dev)
            outs_r[rb, rw] = rr
        else:
            # (a mask round is a launch of few, short units: no row skipping where the library chunks it -- DESIGN.md 4)
            outs_r = torch.stack(pl._scan_jobs(st.dirty, [(self.aidx[a], o_act, l_act, self.hint[a]) for a in range(a0, A)], MODE_TWO_PASS, st.dmax,
                                               sort_lengths=win.ragged, typ_len=st.dtyp, floors=self.floors[a0:] if self.floors is not None else None,
                                               no_skip_underfilled=True))                  # [A - a0, active, 8]
        # (all adapters at once: a loop over the 196 sequences of a barcode panel is ~2 000 tiny launches a round)
        st.rec_all[a0:, act] = outs_r
        st.full_all[a0:, act] = self.glue.middle_hits(outs_r.contiguous(), self.thr)[0]

    def account(self, st):
        pl = self.pl
        pl.stats["pairs_middle"] += st.n_align
        add_stat(pl.stats, "pairs_middle_speculative", st.n_spec)
        add_stat(pl.stats, "pairs_middle_kept_by_mask_rule", st.n_kept)
        if self.floors is not None:
            # (the context's running total, read once per call where the device has just been waited for -- the last round's
            # statistics above, or the dirty-read count -- so the 16-byte copy waits for nothing)
            total = self.al.floor_skipped()[1]
            add_stat(pl.stats, "pairs_middle_skipped_by_floor", total - pl._floor_seen)
            pl._floor_seen = total
