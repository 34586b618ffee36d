"""Batched form of Porechop's three adapter-search phases, driving the GPU library.

This is the host-side mirror of the CALLERS of the hot path, batched so that the GPU sees
millions of (window, adapter) pairs per launch instead of one pair per ctypes call:

  phase A  porechop/porechop.py:286-327   find_matching_adapter_sets (+ nanopore_read.py:149-164)
  phase B  porechop/porechop.py:438-514   find_adapters_at_read_ends (+ nanopore_read.py:166-208)
  phase C  porechop/porechop.py:533-595   find_adapters_in_read_middles (+ nanopore_read.py:210-243)

Every decision (thresholds, trim arithmetic, the sequential mask-and-realign loop of phase C) is
the reference's, evaluated with torch tensor ops on the device from the integer records the
kernels return; the alignments themselves only ever come from the C ABI (no CPU path).
PyTorch is plumbing here: it owns the HBM buffers and the stream.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import math
import os

import numpy as np
import torch

from .batch import MODE_AUTO, MODE_SCORE, MODE_TRACE, MODE_TRACE_AT, MODE_TWO_PASS, NO_FLOOR, Aligner, RESULT_INTS
# the middle scan's glue, its pure helpers and the loop of phase_c live in middle.py; the helpers keep their names here
from .middle import (MiddleHits, MiddleScan, _identities, _round6, add_stat, choose_glue, middle_mask_tables, must_realign_torch,
                     set_positions, switch_on, trimmed_interval)

# phase B is pruned (exactly: see "Exact pruning of phase B" below) from this many (sequence, side) jobs on; measured on
# MI355X, 1 M reads: 198 jobs 192 -> 122 ms; with the 4-6 jobs of a run without barcodes tracing everything is faster
PRUNE_MIN_JOBS = int(os.environ.get("PC_PRUNE_MIN_JOBS", "24"))
# below that, phase B hands its rule to the end-window scan (pc_scan_device_end_rule) from this many reads on.  The route saves
# traced cells per pair and costs six small launches per row class, one class after the other, where the traced-in-full launches
# run two at a time: measured on MI355X with the headline's four jobs, one synchronised phase_b call takes 4.02 ms against 4.60
# at 1 M reads, 2.88 / 2.82 at 600 k, 2.33 / 2.05 at 400 k, 1.46 / 0.82 at 100 k (profiles/end_floor_before_after.txt)
END_RULE_MIN_READS = int(os.environ.get("PC_END_RULE_MIN_READS", "750000"))
# up to this many adapter sets the prefilter stage of the middle scan takes ONE host round trip (survivors counted per set on
# the device); a barcode panel's ~100 sets keep the single compaction over all of them
LEAN_PREFILTER_GROUPS = 8


@dataclass
class AdapterSet:
    """Mirror of porechop/adapters.py:18-52 (name + optional (name, seq) start / end)."""
    name: str
    start: Optional[Tuple[str, str]] = None
    end: Optional[Tuple[str, str]] = None


@dataclass
class ScanParams:
    # defaults of porechop/porechop.py:138-185
    end_size: int = 150
    min_trim_size: int = 4
    extra_end_trim: int = 2
    end_threshold: float = 75.0
    middle_threshold: float = 90.0
    adapter_threshold: float = 90.0
    check_reads: int = 10000
    scores: Tuple[int, int, int, int] = (3, -6, -5, -2)
    # packed-only reads (DeviceReads.packed_only): the prefilter takes EVERY middle-adapter list over the plane
    # (pc_prefilter_packed_any) instead of unpacking all reads for a list the seed stage cannot cover
    packed_total: bool = False
    # IUPAC wildcards in the adapters (Aligner.set_wildcards): off by default
    wildcards: bool = False


@dataclass
class DeviceReads:
    """Reads resident in HBM: one byte per base as delivered (upper-cased ASCII), read r at
    arena[off[r] : off[r] + length[r]].  The arena must have >= 16 readable bytes after the last
    read (the kernels fetch bases a dword at a time)."""
    arena: Optional[torch.Tensor]    # uint8 [bytes]; None = the reads are held PACKED only (plane / exc / ends below)
    off: torch.Tensor      # int64 [R]
    length: torch.Tensor   # int32 [R]
    # reads held at 2 bits per base (packed_only): the plane io.pack_reads makes (base i of the arena in bits 2 (i % 16) of
    # dword i / 16; 64 readable bytes past the last base), the ascending positions of the bases that were not A/C/G/T/U, and
    # byte copies of every read's two end windows: (arena, start window offsets, end window offsets, end_size)
    plane: Optional[torch.Tensor] = None
    exc: Optional[torch.Tensor] = None
    nbases: int = 0
    ends: Optional[tuple] = None

    @property
    def n(self):
        return int(self.off.shape[0])

    @classmethod
    def packed_only(cls, aligner, packed, nbases, exceptions, off, length, end_size=150):
        """Reads that crossed PCIe at 2 bits per base and STAY packed in HBM (a quarter of the bytes): only what the DP kernels
        read is ever turned into bytes -- here the two end windows of every read (pc_unpack_windows: 2 x end_size bytes per
        read), later the few whole reads that survive the exact prefilter, which itself scans the plane
        (pc_prefilter_packed).  off / length index the plane in BASES (the byte offsets of the arena it was packed from)."""
        dev = packed.device
        need = (int(nbases) + 15) // 16 * 4 + 64
        if int(packed.numel()) < need:                         # the scan fetches whole 16-byte blocks: slack past the last base
            grown = torch.zeros(need, dtype=torch.uint8, device=dev)
            grown[:packed.numel()] = packed
            packed = grown
        n = int(off.shape[0])
        ln64 = length.to(torch.int64)
        wl = torch.clamp(length, max=end_size).to(torch.int32).contiguous()
        stride = (end_size + 15) // 16 * 16 + 16
        dst_off = torch.arange(2 * n + 1, dtype=torch.int64, device=dev) * stride
        ends = torch.empty(2 * n * stride + 64, dtype=torch.uint8, device=dev)
        ends[2 * n * stride:] = ord("N")
        if n:
            aligner.unpack_windows(packed, exceptions, off.contiguous(), wl, ends, dst_off[:n + 1].contiguous())
            aligner.unpack_windows(packed, exceptions, (off + (ln64 - wl.to(torch.int64))).contiguous(), wl, ends, dst_off[n:].contiguous())
        return cls(None, off, length, plane=packed, exc=exceptions, nbases=int(nbases),
                   ends=(ends, dst_off[:n], dst_off[n:2 * n], int(end_size)))

    def materialize(self, aligner):
        """The byte arena of packed-only reads (pc_unpack_device), for the routes that need every base as a byte."""
        if self.arena is None:
            self.arena = aligner.unpack_device(self.plane[:(self.nbases + 15) // 16 * 4], self.nbases, self.exc)
        return self.arena

    @classmethod
    def from_packed(cls, aligner, packed, nbases, exceptions, off, length, arena=None):
        """Reads that crossed PCIe at 2 bits per base (io.pack_reads) -> the resident byte arena (pc_unpack_device:
        'A' / 'C' / 'G' / 'T', 'N' at the listed exceptions, 64 bytes of 'N' behind the last read)."""
        return cls(aligner.unpack_device(packed, nbases, exceptions, arena=arena), off, length)


@dataclass
class EndExplain:
    """Why phase B trimmed and called each read as it did (Pipeline.phase_b_explain; the layout of the tensors is that of
    pc_phase_b_explain, include/porechop_amd.h)."""
    summary: torch.Tensor     # int32 [R, 12]   trims, numbers of qualifying alignments, deciding jobs, best / second-best bins
    bscore: torch.Tensor      # float64 [R, 4]  full identities of the four bins of summary[:, 6:10]
    hit_first: torch.Tensor   # int64 [R + 1]   read r's qualifying alignments are hits[hit_first[r] : hit_first[r + 1]]
    hits: torch.Tensor        # int32 [H, 6]    job, read_start, read_end (exclusive), matches, aligned_len, full_len
    jobs: List[Tuple[int, int]] = field(default_factory=list)     # job -> (side: 0 start / 1 end, index into Pipeline.sets)
    bins: Optional[list] = None                                   # the bins the call was made over, or None
    # phase_b_explain(paths=True): the path of every hit, row for row with `hits` (Aligner.align_paths' heads and operations)
    path_heads: Optional[torch.Tensor] = None                     # int32 [H, 4]  path_len, read_first, adapter_first, opens
    path_ops: Optional[torch.Tensor] = None                       # int32 [H, pitch]


def call_barcodes(nbins: int, start_scores: torch.Tensor, end_scores: torch.Tensor, barcode_threshold: float,
                  barcode_diff: float, require_two_barcodes: bool) -> np.ndarray:
    """nanopore_read.py:399-466 for every read at once (torch formulation; the GPU product path runs
    the same rules in pc_phase_b_reduce).

    start_scores / end_scores are float64 [R, K]: the full-adapter identity of bin k's start / end
    sequence (the reference's two dicts, in insertion order; bin names are distinct), NaN where the
    dict has no entry (a bin without that side's set, or an untraced pair).  A missing entry is left
    out of the sorted lists, like the reference's: it is never best or second best, and a side with
    no entry at all is ('none', 0.0).
    -> int64 [R] bin index, or -1 for 'none'.

    Ties are resolved as Python's stable sorted(..., reverse=True) resolves them there: among equal
    scores the entry inserted first wins, start entries before end entries."""
    R, K = start_scores.shape
    dev = start_scores.device
    none = torch.full((R,), -1, dtype=torch.int64, device=dev)
    if K == 0:
        return none.cpu().numpy()       # best = ('none', 0.0): the call is 'none' whatever the thresholds
    start_scores = torch.nan_to_num(start_scores, nan=-math.inf)    # absent: below every identity
    end_scores = torch.nan_to_num(end_scores, nan=-math.inf)

    def best_two(x):
        order = torch.sort(x, dim=1, descending=True, stable=True)
        second = order.values[:, 1] if x.shape[1] >= 2 else torch.zeros(R, dtype=x.dtype, device=dev)
        present = order.values[:, 0] > -math.inf
        return torch.where(present, order.indices[:, 0], none), torch.clamp(order.values[:, 0], min=0.0), torch.clamp(second, min=0.0)

    if require_two_barcodes:
        si, sv, s2 = best_two(start_scores)
        ei, ev, e2 = best_two(end_scores)
        ok = (sv >= barcode_threshold) & (ev >= barcode_threshold) & \
             (sv >= s2 + barcode_diff) & (ev >= e2 + barcode_diff)
        ok &= si == ei                                             # start_end_match compares NAMES (distinct per bin)
        call = torch.where(ok, si, none)
    else:
        both = torch.cat([start_scores, end_scores], dim=1)            # start entries first
        bi, bv, _ = best_two(both)
        bk = torch.where(bi >= 0, bi % K, none)
        # second best = best score among the OTHER names (each name keeps its best of start/end)
        per_name = torch.maximum(start_scores, end_scores)
        other = per_name.masked_fill(torch.arange(K, device=dev)[None, :] == bk[:, None], -1.0)
        second = torch.clamp(other.max(dim=1).values, min=0.0)
        ok = (bk >= 0) & (bv >= barcode_threshold) & (bv >= second + barcode_diff)
        call = torch.where(ok, bk, none)
    return call.cpu().numpy()


class Pipeline:
    def __init__(self, sets: List[AdapterSet], params: ScanParams = None, device=None, aligner=None):
        """aligner: an object with the Aligner interface.  The default -- and the only product
        path -- is the GPU library; tests inject an oracle-backed stand-in to check the host logic
        on machines without a GPU."""
        self.sets = []
        self.p = params or ScanParams()
        self.seq_index = {}
        self.seqs = []
        self._register(sets)
        if aligner is None:
            self.device = torch.device(device if device is not None else "cuda")
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.aligner = Aligner(self.seqs, self.p.scores, device=dev_index, wildcards=self.p.wildcards)
        else:
            self.device = torch.device(device if device is not None else "cpu")
            self.aligner = aligner
            if self.p.wildcards or getattr(aligner, "wildcards", False):
                self.aligner.set_wildcards(self.p.wildcards)      # (an aligner without the mode: an error, not a silent off)
            self.aligner.set_adapters(self.seqs)
        self.stats = {"pairs_end": 0, "pairs_middle": 0, "cells_end": 0, "cells_middle": 0}
        self._floor_seen = 0          # the aligner's total of pairs left untraced by a score floor, as of the last phase_c
        self._consts = {}

    def _const(self, values, dtype=torch.int64):
        """A small read-only device tensor of host values (job -> set / side / adapter length tables ...), kept between calls: a
        torch.tensor(list, device=cuda) is a pageable upload that WAITS for everything enqueued before it -- half a dozen of
        them per step were half a dozen drains of the GPU's queue (0.5 ms each at 1 M reads), for tables that repeat from batch
        to batch."""
        key = (dtype, tuple(values))
        t = self._consts.get(key)
        if t is None:
            if len(self._consts) > 512:
                self._consts.clear()
            t = self._consts[key] = torch.tensor(list(values), dtype=dtype, device=self.device)
        return t

    def packed_kernels(self):
        """True when every pair of this pipeline runs the packed 16-bit kernels (pc_scores_supported): the exact prunings
        below (score bounds, PC_MODE_SCORE records) are derived for those schemes.  Any other scheme -- the reference takes
        any four integers -- and adapters above 128 bases run the library's plain-int32 kernel: same answers, every record
        computed, no pruning."""
        lib = getattr(self.aligner, "lib", None)
        if lib is None or not hasattr(lib, "pc_scores_supported"):
            # test stand-ins (no library): the sign conditions the bounds' derivations rest on
            match, mismatch, go, ge = [int(x) for x in self.p.scores]
            return match > 0 and match > mismatch and go < 0 and ge < 0
        longest = max([len(x) for x in self.seqs] + [1])
        return bool(lib.pc_scores_supported(*[int(x) for x in self.p.scores], int(longest)))

    def _register(self, sets):
        # one adapter table for everything (deduplicated sequences)
        for s in sets:
            self.sets.append(s)
            for side in (s.start, s.end):
                if side is not None and side[1] not in self.seq_index:
                    self.seq_index[side[1]] = len(self.seqs)
                    self.seqs.append(side[1])

    def add_sets(self, sets: List[AdapterSet]) -> List[int]:
        """Append adapter sets found necessary after phase A (porechop.py:410-436: the full barcode
        adapters) -> their indices in self.sets."""
        first = len(self.sets)
        self._register(sets)
        self.aligner.set_adapters(self.seqs)
        return list(range(first, len(self.sets)))

    # ------------------------------------------------------------------------------------------
    def _end_windows(self, reads: DeviceReads, idx: Optional[torch.Tensor], side: str):
        """seq[:end_size] / seq[-end_size:] as (offset, length) windows (nanopore_read.py:155,160)."""
        ln = reads.length if idx is None else reads.length[idx]
        wl = torch.clamp(ln, max=self.p.end_size)
        if reads.arena is None:                      # packed-only reads: the windows' byte copies (DeviceReads.packed_only)
            assert reads.ends is not None and reads.ends[3] == self.p.end_size
            tab = reads.ends[1] if side == "start" else reads.ends[2]
            return (tab if idx is None else tab[idx]), wl
        off = reads.off if idx is None else reads.off[idx]
        if side == "start":
            return off, wl
        return off + (ln - wl).to(torch.int64), wl

    @staticmethod
    def _ends_arena(reads: DeviceReads):
        """The bytes the end windows index: the read arena, or -- packed-only reads -- the copies of the end windows."""
        return reads.arena if reads.arena is not None else reads.ends[0]

    def _scan_jobs(self, arena, jobs, mode, max_len, with_layout=False, sort_lengths=False, typ_len=0, fuse=True, floors=None,
                   end_sides=None, presorted=False, no_skip_underfilled=False):
        """jobs: list of (adapter_index, win_off int64[n], win_len int32[n]) -> list of [n,8] views.

        floors (MODE_TWO_PASS): one score per job -- a pair whose best score is below it is not traced and gets the
        "no alignment" record (-1, 0, ..., 0), decided in the library between its two passes (Aligner.scan_device).
        end_sides (MODE_AUTO over end windows): one side per job, 0 = start windows, 1 = end windows -- a pair that cannot trim
        its read by phase B's rule (this pipeline's end_size, min_trim_size, extra_end_trim, end_threshold) gets that same
        record instead of a traceback, decided in the same place.

        Jobs that scan the very same windows (same tensors) are fused two adapters at a time
        (similar lengths together), so each window is streamed from HBM once per adapter PAIR.

        sort_lengths: whole-read scans of reads of different lengths.  A tile (64 or 128 consecutive
        windows) runs as many columns as its longest window, so the windows of every job are handed
        over longest first -- a tile then holds windows of nearly one length, and the specialised score
        kernel stays on its block-resolved path -- and the records are put back in the caller's order.
        typ_len: their typical (mean) length, which lets the library cut the longest reads into chunks of
        about that many columns (pc_set_length_hint) so that a launch does not last as long as its longest read.
        presorted: such windows, which the caller already hands over longest first (typ_len as above; nothing is reordered).
        no_skip_underfilled: Aligner.scan_device's option of that name, for this call.  It means something with floors only
        (an unfloored call skips no rows anyway) and is dropped without them."""
        order_of = {}
        if sort_lengths:
            sorted_jobs = []
            for j in jobs:
                key = (id(j[1]), id(j[2]))
                if key not in order_of:
                    order = torch.argsort(j[2], descending=True, stable=True)
                    order_of[key] = (order, j[1][order], j[2][order], j[1], j[2])   # keeps the originals alive (ids stay unique)
                sorted_jobs.append((j[0], order_of[key][1], order_of[key][2]) + tuple(j[3:]))
            orders = [order_of[(id(j[1]), id(j[2]))][0] for j in jobs]
            jobs = sorted_jobs
        if switch_on("PC_NO_FUSE"):        # (timing experiments: every adapter alone, exact rows, two read streams)
            fuse = False
        groups = {}
        for k, j in enumerate(jobs):
            # fuse=False: every job alone (one adapter per kernel: the single-sequence kernels ship with the library)
            groups.setdefault((id(j[1]), id(j[2])) if fuse else k, []).append(k)
        fused = []                      # (job index a, job index b or None)
        for ks in groups.values():
            # jobs that carry the same pairing hint (the two sequences of one adapter set, phase C) go together,
            # longer adapter first: a set's pair is the same in every run, so its specialised score kernel can
            # be -- and for the static panel is -- built ahead of time (porechop_amd/aot.py)
            by_hint, rest = {}, []
            for k in ks:
                h = jobs[k][3] if len(jobs[k]) > 3 else None
                if h is None:
                    rest.append(k)
                else:
                    by_hint.setdefault(h, []).append(k)
            for h, hk in by_hint.items():
                if isinstance(h, tuple) and h and h[0] == "alone":
                    fused.extend((k, None) for k in hk)           # scanned with its single-sequence kernel
                elif len(hk) == 2 and self.seqs[jobs[hk[0]][0]] != self.seqs[jobs[hk[1]][0]]:
                    a, b = hk
                    fused.append((a, b) if len(self.seqs[jobs[a][0]]) >= len(self.seqs[jobs[b][0]]) else (b, a))
                else:
                    rest.extend(hk)
            ks = sorted(rest, key=lambda k: -len(self.seqs[jobs[k][0]]))
            for i in range(0, len(ks) - 1, 2):
                fused.append((ks[i], ks[i + 1]))
            if len(ks) % 2:
                fused.append((ks[-1], None))
        woff = torch.cat([jobs[a][1] for a, _ in fused])
        wlen = torch.cat([jobs[a][2] for a, _ in fused]).to(torch.int32)
        starts = np.zeros(len(fused) + 1, dtype=np.int64)
        ostarts = np.zeros(len(fused) + 1, dtype=np.int64)
        for k, (a, b) in enumerate(fused):
            n = jobs[a][1].shape[0]
            starts[k + 1] = starts[k] + n
            ostarts[k + 1] = ostarts[k] + n * (2 if b is not None else 1)
        out = torch.empty((int(ostarts[-1]), RESULT_INTS), dtype=torch.int32, device=self.device)
        if starts[-1] > 0:
            self.aligner.set_length_hint(typ_len if sort_lengths or presorted else 0)
            fl = {}
            if floors is not None:
                fl = dict(floors=np.array([floors[a] for a, _ in fused], dtype=np.int32),
                          floors_b=np.array([floors[b] if b is not None else NO_FLOOR for _, b in fused], dtype=np.int32))
                if no_skip_underfilled:
                    fl["no_skip_underfilled"] = True
            if end_sides is not None:
                p = self.p
                fl = dict(end_rule=(p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold),
                          job_side=np.array([end_sides[a] for a, _ in fused], dtype=np.int32))
            self.aligner.scan_device(arena, woff, wlen, np.array([jobs[a][0] for a, _ in fused], dtype=np.int32),
                                     starts, max_len, out, mode,
                                     job_adapter_b=np.array([jobs[b][0] if b is not None else -1 for _, b in fused],
                                                            dtype=np.int32), **fl)
        res = [None] * len(jobs)
        rec_off = [0] * len(jobs)
        for k, (a, b) in enumerate(fused):
            n = jobs[a][1].shape[0]
            o = int(ostarts[k])
            res[a] = out[o:o + n]; rec_off[a] = o
            if b is not None:
                res[b] = out[o + n:o + 2 * n]; rec_off[b] = o + n
        if sort_lengths:
            assert not with_layout
            back = []
            for r, order in zip(res, orders):
                u = torch.empty_like(r)
                u[order] = r
                back.append(u)
            return back
        if with_layout:
            return res, out, rec_off          # + the one tensor behind the views and each job's first record
        return res

    # ------------------------------------------------------------------------------------------
    def presence_score_bound(self, m: int) -> Optional[int]:
        return self.identity_score_bound(m, self.p.adapter_threshold)

    def identity_score_bound(self, m: int, threshold: float) -> Optional[int]:
        """Smallest raw score an alignment of an m-base adapter can have if its full-adapter identity
        reaches `threshold` percent (None when the scheme gives no bound).  With t = threshold/100:
        identity >= t means matches M >= t * L_full >= t * m and non-match columns N <= M (1-t)/t;
        every scored non-match column costs at most P = max(|mismatch|, |gap_open|, |gap_extend|) and
        overhanging adapter bases cost nothing, so score >= match*M - P*N >= m * (t*match - P*(1-t))."""
        match, mismatch, go, ge = self.p.scores
        t = (threshold - 1e-6) / 100.0                          # the identity is compared after %f rounding
        per_base = t * match - max(-mismatch, -go, -ge) * (1.0 - t)
        if per_base <= 0:
            return None
        return int(np.floor(m * per_base))

    def phase_a(self, reads: DeviceReads, check_idx: Optional[torch.Tensor] = None, prune: bool = False):
        """-> (best_start[S], best_end[S]) float64 on device: the max full-adapter identity of every
        set's start / end sequence over the check reads.  This table is the only cross-read
        reduction in Porechop (nanopore_read.py:159,164); a multi-GPU run all-reduces it (MAX).

        prune=True: a score-only pass first, then traceback only for the pairs whose
        score can still mean an identity >= --adapter_threshold (presence_score_bound).  Which sets
        reach the threshold, and their best identities, are exactly the unpruned ones; the table
        entries of sets that do NOT reach it become lower bounds (they only feed a display in the
        reference), which is why this is an option and not the default."""
        S = len(self.sets)
        best_start = torch.zeros(S, dtype=torch.float64, device=self.device)
        best_end = torch.zeros(S, dtype=torch.float64, device=self.device)
        n = reads.n if check_idx is None else int(check_idx.shape[0])
        if n == 0:
            return best_start, best_end
        so, sl = self._end_windows(reads, check_idx, "start")
        eo, el = self._end_windows(reads, check_idx, "end")
        jobs, where = [], []
        for si, s in enumerate(self.sets):
            if "(full sequence)" in s.name:       # porechop.py:296
                continue
            if s.start is not None:
                jobs.append((self.seq_index[s.start[1]], so, sl)); where.append((si, 0))
            if s.end is not None:
                jobs.append((self.seq_index[s.end[1]], eo, el)); where.append((si, 1))
        if prune and self.packed_kernels():
            return self._phase_a_pruned(reads, jobs, where, best_start, best_end)
        outs = self._scan_jobs(self._ends_arena(reads), jobs, MODE_TRACE, self.p.end_size)
        # one vectorised reduction for all jobs (they all cover the same n check reads)
        rec = torch.stack(outs)                                     # [J, n, 8]
        m = rec[:, :, 5].to(torch.float64)
        full = _round6(100.0 * m / rec[:, :, 7].to(torch.float64))
        full = torch.where(rec[:, :, 0] == -1, torch.zeros_like(full), full).amax(dim=1)   # [J]
        # (which job feeds which entry is known on the host: index lists, not boolean masks -- a mask is a nonzero, a round trip)
        for side, best in ((0, best_start), (1, best_end)):
            ks = [k for k, w in enumerate(where) if w[1] == side]
            if ks:
                best.scatter_reduce_(0, self._const([where[k][0] for k in ks]), full[self._const(ks)], reduce="amax")
        self.stats["pairs_end"] += sum(int(j[1].shape[0]) for j in jobs)
        return best_start, best_end

    def _phase_a_pruned(self, reads, jobs, where, best_start, best_end):
        scores = torch.stack(self._scan_jobs(self._ends_arena(reads), jobs, MODE_SCORE, self.p.end_size))[:, :, 4]   # [J, n]
        bounds = [self.presence_score_bound(len(self.seqs[j[0]])) for j in jobs]
        need = self._const([b if b is not None else -(1 << 30) for b in bounds])
        cand = scores >= need[:, None]
        hit = torch.nonzero(cand)                              # [C, 2] (job, window), job-major: one sync
        counts = torch.bincount(hit[:, 0], minlength=len(jobs)).cpu().numpy()
        cjobs, cwhere = [], []
        pos = 0
        for k, (j, w) in enumerate(zip(jobs, where)):
            if counts[k]:
                sel = hit[pos:pos + int(counts[k]), 1]
                pos += int(counts[k])
                cjobs.append((j[0], j[1][sel], j[2][sel])); cwhere.append(w)
        self.stats["pairs_end"] += sum(int(j[1].shape[0]) for j in jobs)
        add_stat(self.stats, "pairs_end_traced_after_pruning", int(counts.sum()))
        if not cjobs:
            return best_start, best_end
        outs = self._scan_jobs(self._ends_arena(reads), cjobs, MODE_TRACE, self.p.end_size)
        rec = torch.cat(outs)                                   # one reduction for all candidate jobs
        full, _ = _identities(rec)
        full = torch.where(rec[:, 0] == -1, torch.zeros_like(full), full)
        job_of = torch.repeat_interleave(torch.arange(len(cjobs), device=self.device),
                                         torch.tensor([int(j[1].shape[0]) for j in cjobs], device=self.device))
        top = torch.zeros(len(cjobs), dtype=torch.float64, device=self.device).scatter_reduce_(0, job_of, full, reduce="amax")
        for side, best in ((0, best_start), (1, best_end)):
            ks = [k for k, w in enumerate(cwhere) if w[1] == side]
            if ks:
                best.scatter_reduce_(0, self._const([cwhere[k][0] for k in ks]), top[self._const(ks)], reduce="amax")
        return best_start, best_end

    def matching_sets(self, best_start, best_end):
        """porechop.py:327: sets whose best start-or-end score reaches --adapter_threshold."""
        best = torch.maximum(best_start, best_end).cpu().numpy()
        return [i for i, s in enumerate(self.sets)
                if "(full sequence)" not in s.name and best[i] >= self.p.adapter_threshold]

    # ------------------------------------------------------------------------------------------
    def _phase_b_jobs(self, reads, matching):
        so, sl = self._end_windows(reads, None, "start")
        eo, el = self._end_windows(reads, None, "end")
        jobs, where = [], []
        for si in matching:
            s = self.sets[si]
            if s.start is not None:
                jobs.append((self.seq_index[s.start[1]], so, sl)); where.append((0, si))
            if s.end is not None:
                jobs.append((self.seq_index[s.end[1]], eo, el)); where.append((1, si))
        return jobs, where

    def umi_adapters(self, matching):
        """[(side, set index, adapter index, (u0, u1))] for the start (side 0) and end (side 1) sequences of the `matching`
        sets that have a UMI span (Aligner.umi_span: a row whose letter stands for two or more bases), in matching order."""
        if not getattr(self.aligner, "umi", False):
            raise RuntimeError("this aligner extracts no UMIs (Aligner.umis)")
        out = []
        for si in matching:
            s = self.sets[si]
            for side, ad in ((0, s.start), (1, s.end)):
                if ad is not None:
                    ai = self.seq_index[ad[1]]
                    span = self.aligner.umi_span(ai)
                    if span is not None:
                        out.append((side, si, ai, span))
        return out

    def end_umis(self, reads: DeviceReads, matching: List[int]):
        """The UMI of every read's start and end: the read bases under the degenerate rows of the matching sets' adapters
        (DESIGN.md section 16).  One Aligner.umis call per UMI adapter over the end windows of its side, under phase B's
        rule (this pipeline's end_size, min_trim_size, extra_end_trim, end_threshold); per read and side the complete
        extraction (status 0) with the highest alignment score is kept, ties going to the adapter that comes first in
        `matching`.  -> [(set, first, length, covered) for the start side, the same for the end side], int32[R] device
        tensors each: set = index into self.sets, -1 where the read has no UMI on that side; first = the UMI's first base in
        WHOLE-READ coordinates (-1 without one); covered = span rows aligned to a read base."""
        R = reads.n
        p = self.p
        dev = self.device
        rule = (p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold)
        adapters = self.umi_adapters(matching)
        self.stats.setdefault("umi_pairs", 0)
        out = []
        for side, name in ((0, "start"), (1, "end")):
            best_set = torch.full((R,), -1, dtype=torch.int32, device=dev)
            best_score = torch.zeros(R, dtype=torch.int32, device=dev)
            best = torch.zeros((R, 3), dtype=torch.int32, device=dev)
            best[:, 0] = -1
            mine = [a for a in adapters if a[0] == side]
            if R and mine:
                off, wl = self._end_windows(reads, None, name)
                off, wl = off.to(torch.int64).contiguous(), wl.to(torch.int32).contiguous()
                for _, si, ai, _span in mine:
                    recs, umi = self.aligner.umis(self._ends_arena(reads), off, wl, ai, side, rule=rule, max_len=p.end_size)
                    add_stat(self.stats, "umi_pairs", R)
                    better = (umi[:, 0] == 0) & ((best_set < 0) | (recs[:, 4] > best_score))      # strict: the earlier adapter keeps a tie
                    best_set = torch.where(better, torch.full_like(best_set, si), best_set)
                    best_score = torch.where(better, recs[:, 4], best_score)
                    best = torch.where(better[:, None], umi[:, 1:4], best)
                if side == 1:                          # window columns -> read coordinates
                    shift = (reads.length.to(torch.int32) - wl)
                    best[:, 0] = torch.where(best[:, 0] >= 0, best[:, 0] + shift, best[:, 0])
            out.append((best_set, best[:, 0].contiguous(), best[:, 1].contiguous(), best[:, 2].contiguous()))
        return out

    @property
    def native_reduce(self):
        """The per-read reduction of phase B runs as a library kernel (pc_phase_b_reduce) on the GPU;
        an injected test aligner without it takes the equivalent torch formulation below."""
        return hasattr(self.aligner, "phase_b_reduce")

    # ------------------------------------------------------------------------------------------
    # Exact pruning of phase B.  Of the ~200 end-window alignments a barcoded read gets, three matter: phase B keeps the
    # MAXIMUM trim over the alignments that qualify (nanopore_read.py:166-208) and the barcode call looks at full
    # identities within --barcode_diff of the best (nanopore_read.py:399-466).  A score-only pass (5 instead of 13.25
    # packed ops per two cells, no trace slab) gives every alignment's end cell (I adapter bases and Jc window columns
    # consumed) and score S -- the reference's own end cell, the one the two-pass scan retraces -- and from those,
    # UPPER BOUNDS on what the alignment can contribute:
    #   full identity <= 100 min(I, Jc, m) / m              (matches <= diagonal columns <= bases consumed; span >= m)
    #   start window:  read_end <= Jc + 1, so trim <= Jc + 1 + extra; none if Jc + 1 < min_trim_size; none if the path ends
    #                  in the window's last column of a full window (then read_end == end_size, which disqualifies)
    #   end window:    a qualifying alignment starts on the first row at a column j0 >= 1 (read_start = j0; a path from the
    #                  first column has read_start 0, which disqualifies), consumes all I adapter bases and b = Jc - j0 window
    #                  columns with  S <= (match + g) b - g I  and  b <= I + (match I - S) / g,  g = min(|open|, |extend|);
    #                  so none if Jc - 1 < ceil((S + g I) / (match + g)), else trim <= end_size - max(1, Jc - bmax) + extra.
    #   either side:   a qualifying alignment has aligned identity > --end_threshold over Lp >= min(I, Jc) columns, hence
    #                  S > (tau match - (1 - tau) P) min(I, Jc)   (P = the dearest non-matching column)
    # Round 1 traces, per read and side, the two best-scoring pairs that can trim at all and the two best-scoring barcode
    # pairs; the exact reduction of those gives each read's trims so far and the best barcode identity per side; round 2 traces
    # the pairs whose trim bound still exceeds the trims, and the barcode pairs that could reach
    # max(best, --barcode_threshold) - --barcode_diff (a full identity of t also needs S >= m (t match - (1 - t) P)).
    # Every pair left untraced is proven unable to change the maximum
    # or the call and enters the reduction as "no alignment".  tests/test_gpu_phase_b_pruning.py checks the bounds against
    # the full records of EVERY pair of its batches and the results against the unpruned phase B.
    def _phase_b_bounds(self, score_rec, jobs, where, sl, el):
        """score_rec [J, R, 8] (MODE_SCORE records) -> (ub_trim int64 [J, R], ub_full float64 [J, R])."""
        p = self.p
        dev = self.device
        match, _, go, ge = p.scores
        g = min(-go, -ge)
        m = self._const([len(self.seqs[j[0]]) for j in jobs])[:, None]
        is_end = self._const([bool(w[0]) for w in where], torch.bool)[:, None]
        n = torch.where(is_end, el[None, :].to(torch.int64), sl[None, :].to(torch.int64))
        flag = score_rec[:, :, 0].to(torch.int64)
        Jc = score_rec[:, :, 1].to(torch.int64)
        I = score_rec[:, :, 2].to(torch.int64)
        S = score_rec[:, :, 4].to(torch.int64)
        ub_full = 100.0 * torch.minimum(torch.minimum(I, Jc), m).to(torch.float64) / m.to(torch.float64)
        # start windows
        ok_s = (Jc + 1 >= p.min_trim_size) & ~((Jc == n) & (n == p.end_size))
        ub_s = torch.where(ok_s, Jc + 1 + p.extra_end_trim, torch.zeros_like(Jc))
        # end windows
        bmin = torch.div(S + g * I + (match + g - 1), match + g, rounding_mode="floor")
        bmax = I + torch.div(torch.clamp(match * I - S, min=0), g, rounding_mode="floor")
        ok_e = (Jc - 1 >= bmin) & (bmax + 1 >= p.min_trim_size)
        ub_e = torch.where(ok_e, p.end_size - torch.clamp(Jc - bmax, min=1) + p.extra_end_trim, torch.zeros_like(Jc))
        ub = torch.where(is_end, ub_e, ub_s)
        # either side: a trim needs aligned identity > --end_threshold over the path's Lp columns, Lp >= min(I, Jc) (a path
        # from the first row consumes all I adapter bases, one from the first column all Jc window columns); with
        # M > tau Lp matches and fewer than (1 - tau) Lp other columns at a cost of at most P each,
        # S > (tau match - (1 - tau) P) Lp.  (Random 24-28-mers align into a full window at ~64 % identity with S = 7..17:
        # this is what prunes them.)
        tau = (p.end_threshold - 1e-6) / 100.0
        P = max(-p.scores[1], -go, -ge, 0)
        c = tau * match - (1.0 - tau) * P
        if c > 0:
            need_s = torch.floor(c * torch.clamp(torch.minimum(I, Jc), min=1).to(torch.float64)).to(torch.int64)
            ub = torch.where(S > need_s, ub, torch.zeros_like(ub))
        # and a full identity of t needs S >= m (t match - (1 - t) P)  (identity_score_bound, as in phase A's pruning)
        odd = flag != -2                                   # anything that is not a plain score record: trace it
        ub = torch.where(odd, torch.full_like(ub, 1 << 20), ub)
        ub_full = torch.where(odd, torch.full_like(ub_full, 100.0), ub_full)
        return ub, ub_full

    def _phase_b_pruned_records(self, reads, jobs, where, call_sets, call_level, reduce_trims, call_level_diff=0.0):
        """Records of phase B with only the pairs that can matter traced (see above); the others keep their score-only
        record, which the reduction reads as "no alignment".  call_sets: set indices whose full identities feed a barcode
        call (traced whenever they can reach call_level = threshold - diff, or come within call_level_diff of the best
        traced on their side).  reduce_trims(records, rec_off) -> (start_trim, end_trim) runs the exact reduction.
        The selection runs on the device (pc_select.hip); the host reads back one count per job and round.
        self.debug_bounds (tests): a dict that receives the bounds and the untouched score records.
        -> (records, rec_off); self._traced_mask = the pairs that hold a traced record (int64 [J, words])"""
        p = self.p
        dev = self.device
        al = self.aligner
        self._traced_mask = None
        bounds_out = getattr(self, "debug_bounds", None)
        R, J = reads.n, len(jobs)
        so, sl = self._end_windows(reads, None, "start")
        eo, el = self._end_windows(reads, None, "end")
        so, eo = so.contiguous(), eo.contiguous()
        sl, el = sl.to(torch.int32).contiguous(), el.to(torch.int32).contiguous()
        # barcodes 2k-1 and 2k of a direction share a pass over their windows (one read stream instead of two: 10 instead
        # of 8 TCUPS), every other sequence runs alone; both kinds of kernel ship with the library (porechop_amd/aot.py)
        from . import panel as rules
        hinted = []
        for k, (j, (side, si)) in enumerate(zip(jobs, where)):
            key = rules.phase_b_pair_key(self.sets[si])
            hinted.append(tuple(j[:3]) + ((("pair", side) + key) if key is not None else ("alone", k),))
        _, rec, rec_off = self._scan_jobs(self._ends_arena(reads), hinted, MODE_SCORE, p.end_size, with_layout=True)
        job_off = self._const(rec_off)
        job_side = self._const([w[0] for w in where], torch.int32)
        job_len = self._const([len(self.seqs[j[0]]) for j in jobs], torch.int32)
        job_calls = self._const([1 if w[1] in call_sets else 0 for w in where], torch.int32)
        job_adapter = np.array([j[0] for j in jobs], dtype=np.int32)
        words = (R + 63) // 64
        best_full = torch.zeros((2, R), dtype=torch.float64, device=dev)   # best traced full identity of a call pair, per side
        trace_at = getattr(al, "trace_at", False) and not switch_on("PC_NO_TRACE_AT")

        def trace(mask, counts):
            cnt = counts.cpu().numpy()                                   # the round's one host round trip
            total = int(cnt.sum())
            if total == 0:
                return 0
            first = torch.cumsum(counts, 0) - counts
            woff = torch.empty(total, dtype=torch.int64, device=dev)
            wlen = torch.empty(total, dtype=torch.int32, device=dev)
            dest = torch.empty(total, dtype=torch.int64, device=dev)
            pjob = torch.empty(total, dtype=torch.int32, device=dev)
            pread = torch.empty(total, dtype=torch.int64, device=dev)
            cursor = torch.empty(J, dtype=torch.int64, device=dev)
            al.phase_b_gather(mask, R, first, cursor, job_off, job_side, so, sl, eo, el, woff, wlen, dest, pjob, pread)
            live = np.nonzero(cnt)[0]
            starts = np.zeros(len(live) + 1, dtype=np.int64)
            starts[1:] = np.cumsum(cnt[live])
            al.set_length_hint(0)
            if trace_at:
                # the end cell of every selected pair is known from its score record: only the columns its path can occupy
                # are traced (PC_MODE_TRACE_AT: the second pass of the whole-read scan, for end windows)
                traced = al.gather_records(rec, dest) if hasattr(al, "gather_records") else rec.index_select(0, dest)
                # (the library takes the pairs of a job by end column -- bucket_pairs -- so that a tile runs as many columns as
                # its LATEST end cell needs: adapters found at the start of their windows, J ~ 30 of 150, share tiles)
                al.scan_device(self._ends_arena(reads), woff, wlen, job_adapter[live], starts, p.end_size, traced, MODE_TRACE_AT)
            else:
                traced = torch.empty((total, RESULT_INTS), dtype=torch.int32, device=dev)
                al.scan_device(self._ends_arena(reads), woff, wlen, job_adapter[live], starts, p.end_size, traced, MODE_TRACE)
            al.phase_b_scatter(traced, dest, pjob, pread, rec, job_side, job_calls, best_full, R)
            return total

        def select(rnd, mask_prev=None, trims=(None, None)):
            mask = torch.empty((J, words), dtype=torch.int64, device=dev)
            counts = torch.empty(J, dtype=torch.int64, device=dev)
            ub_t = ub_f = None
            if rnd == 1 and bounds_out is not None:
                ub_t = torch.empty((J, R), dtype=torch.int32, device=dev)
                ub_f = torch.empty((J, R), dtype=torch.float64, device=dev)
                bounds_out.update(ub_trim=ub_t, ub_full=ub_f, score_records=rec.clone(), rec_off=list(rec_off))
            al.phase_b_select(rec, R, job_off, job_side, job_len, job_calls, sl, el, p.end_size, p.min_trim_size,
                              p.extra_end_trim, p.end_threshold, rnd, call_level, call_level_diff, mask, counts,
                              mask_prev=mask_prev, start_trim=trims[0], end_trim=trims[1], best_full=best_full,
                              ub_trim_out=ub_t, ub_full_out=ub_f)
            return mask, counts

        # round 1: per read and side the two best-SCORING pairs that can trim at all (the real adapter and the real barcode,
        # where the read has them) and the two best-scoring barcode pairs (they fix the level a rival would have to reach)
        mask1, counts1 = select(1)
        n1 = trace(mask1, counts1)
        st1, et1 = reduce_trims(rec, rec_off, mask1)
        # round 2: whatever could still beat the trims so far or change the call
        mask2, counts2 = select(2, mask_prev=mask1, trims=(st1, et1))
        n2 = trace(mask2, counts2)
        self.stats["pairs_end"] += J * R
        add_stat(self.stats, "pairs_end_traced_after_pruning", n1 + n2)
        # which pairs hold a traced record: the reductions skip the others without loading them (pc_phase_b_reduce_masked)
        self._traced_mask = torch.bitwise_or(mask1, mask2)
        return rec, rec_off

    def _masked_kw(self, mask):
        """Keyword for phase_b_reduce: the traced-pairs mask, where the aligner's reduction takes one (the GPU library's does)."""
        if mask is None or not getattr(self.aligner, "reduce_takes_mask", False) or switch_on("PC_NO_REDUCE_MASK"):
            return {}
        return {"traced_mask": mask.contiguous()}

    @property
    def can_prune_phase_b(self):
        """Needs the reduction and selection kernels and score records that carry the end cell (the GPU library's do)."""
        return self.native_reduce and hasattr(self.aligner, "phase_b_select") and getattr(self.aligner, "score_end_cell", False) and \
            self.packed_kernels()

    @property
    def can_rule_phase_b(self):
        """Phase B hands its rule to the scan (Aligner.scan_device(end_rule=...)): needs the library's reduction, the packed
        kernels for every pair and an aligner that offers the call.  PC_NO_END_FLOOR=1 switches it off."""
        return self.native_reduce and getattr(self.aligner, "end_rule", False) and hasattr(self.aligner, "floor_skipped") and \
            self.packed_kernels() and not switch_on("PC_NO_END_FLOOR")

    def _prune_b(self, prune, njobs):
        """prune=None: the exact pruning of phase B where it pays -- a barcode panel's worth of jobs (with a handful of
        adapters the score pass, two selections and two host round trips cost more than tracing everything)."""
        if prune is None:
            return self.can_prune_phase_b and njobs >= PRUNE_MIN_JOBS
        return bool(prune) and self.can_prune_phase_b

    def phase_b_demux(self, reads: DeviceReads, matching: List[int], bins, barcode_threshold, barcode_diff, require_two,
                      prune: Optional[bool] = None):
        """Phase B of a demultiplexing run: trims + the barcode call of every read.
        bins: one (start set index or None, end set index or None) per barcode bin, in the order the
        reference inserts the names into its score dicts (nanopore_read.py:185-187,206-208)
        -> (start_trim, end_trim int32[R], call: numpy int64[R], bin index or -1 = 'none')."""
        R = reads.n
        p = self.p
        if not self.native_reduce:
            full_for = {i for b in bins for i in b if i is not None}
            out = self.phase_b(reads, matching, full_for=full_for)
            fulls = out[2] if full_for else {}
            absent = torch.full((R,), math.nan, dtype=torch.float64, device=self.device)
            S = [fulls.get((b[0], 0), absent) if b[0] is not None else absent for b in bins]
            E = [fulls.get((b[1], 1), absent) if b[1] is not None else absent for b in bins]
            S = torch.stack(S, dim=1) if bins else torch.zeros((R, 0), dtype=torch.float64, device=self.device)
            E = torch.stack(E, dim=1) if bins else torch.zeros((R, 0), dtype=torch.float64, device=self.device)
            return out[0], out[1], call_barcodes(len(bins), S, E, barcode_threshold, barcode_diff, require_two)
        start_trim = torch.zeros(R, dtype=torch.int32, device=self.device)
        end_trim = torch.zeros(R, dtype=torch.int32, device=self.device)
        call = torch.full((R,), -1, dtype=torch.int32, device=self.device)
        jobs, where = self._phase_b_jobs(reads, matching)
        masked = self._masked_kw
        tmask = None
        if jobs and R:
            sides = [w[0] for w in where]
            if self._prune_b(prune, len(jobs)):
                def trims(records, offs, mask=None):
                    a = torch.zeros(R, dtype=torch.int32, device=self.device)
                    b = torch.zeros(R, dtype=torch.int32, device=self.device)
                    self.aligner.phase_b_reduce(records, R, offs, sides, p.end_size, p.min_trim_size, p.extra_end_trim,
                                                p.end_threshold, a, b, **masked(mask))
                    return a, b
                call_sets = {i for b in bins for i in b if i is not None}
                out, rec_off = self._phase_b_pruned_records(reads, jobs, where, call_sets, barcode_threshold - barcode_diff, trims,
                                                            call_level_diff=barcode_diff)
                tmask = self._traced_mask
            else:
                _, out, rec_off = self._scan_jobs(self._ends_arena(reads), jobs, MODE_TRACE, p.end_size, with_layout=True)
                self.stats["pairs_end"] += sum(int(j[1].shape[0]) for j in jobs)
            job_of = {(si, side): k for k, (side, si) in enumerate(where)}
            jb = [(job_of.get((b[0], 0), -1) if b[0] is not None else -1,
                   job_of.get((b[1], 1), -1) if b[1] is not None else -1) for b in bins]
            self.aligner.phase_b_reduce(out, R, rec_off, sides, p.end_size, p.min_trim_size, p.extra_end_trim,
                                        p.end_threshold, start_trim, end_trim, bins=jb if bins else None,
                                        barcode_threshold=barcode_threshold, barcode_diff=barcode_diff,
                                        require_two=require_two, call=call, **masked(tmask))
        return start_trim, end_trim, call.to(torch.int64).cpu().numpy()

    def phase_b(self, reads: DeviceReads, matching: List[int], full_for=(), prune: Optional[bool] = None,
                end_rule: Optional[bool] = None):
        """-> (start_trim[R], end_trim[R]) int32: nanopore_read.py:166-208 for every read.
        full_for: set indices whose full-adapter identities are wanted too (barcode calling,
        nanopore_read.py:185-187,206-208) -> third result {(set, side): float64[R]}, side 0 = start.
        end_rule (where the pruned route is not taken): None = the rule goes down to the scan where it pays, from
        END_RULE_MIN_READS reads on; True / False = always / never (always: as far as can_rule_phase_b allows)."""
        R = reads.n
        p = self.p
        start_trim = torch.zeros(R, dtype=torch.int32, device=self.device)
        end_trim = torch.zeros(R, dtype=torch.int32, device=self.device)
        jobs, where = self._phase_b_jobs(reads, matching)
        fulls = {}
        if not jobs:
            return (start_trim, end_trim, fulls) if full_for else (start_trim, end_trim)
        masked = self._masked_kw
        tmask = None
        if self.native_reduce and not full_for and R:
            sides = [w[0] for w in where]
            pruned_b = self._prune_b(prune, len(jobs))
            ruled_b = not pruned_b and self.can_rule_phase_b and (R >= END_RULE_MIN_READS if end_rule is None else bool(end_rule))
            if pruned_b:
                def trims(records, offs, mask=None):
                    a = torch.zeros(R, dtype=torch.int32, device=self.device)
                    b = torch.zeros(R, dtype=torch.int32, device=self.device)
                    self.aligner.phase_b_reduce(records, R, offs, sides, p.end_size, p.min_trim_size, p.extra_end_trim,
                                                p.end_threshold, a, b, **masked(mask))
                    return a, b
                out, rec_off = self._phase_b_pruned_records(reads, jobs, where, set(), 1e9, trims)
                tmask = self._traced_mask
            elif ruled_b:
                # The library scans every window score-only, keeps the pairs that phase B's rule proves unable to trim out of
                # the traced pass and answers them with the "no alignment" record, which is "no trim" in the reduction
                # (pc_scan_device_end_rule; PC_NO_END_FLOOR=1: every pair traced, as below).  Every job alone: the
                # single-sequence score kernels ship with the library and run 150-column windows as fast as a pair's kernel.
                ruled = [tuple(j[:3]) + (("alone", k),) for k, j in enumerate(jobs)]
                _, out, rec_off = self._scan_jobs(self._ends_arena(reads), ruled, MODE_AUTO, p.end_size, with_layout=True, end_sides=sides)
                self.stats["pairs_end"] += sum(int(j[1].shape[0]) for j in jobs)
            else:
                _, out, rec_off = self._scan_jobs(self._ends_arena(reads), jobs, MODE_TRACE, p.end_size, with_layout=True)
                self.stats["pairs_end"] += sum(int(j[1].shape[0]) for j in jobs)
            self.aligner.phase_b_reduce(out, R, rec_off, sides, p.end_size, p.min_trim_size, p.extra_end_trim,
                                        p.end_threshold, start_trim, end_trim, **masked(tmask))
            if ruled_b:
                # (the pairs of this call alone; phase C waits for the trims in its first lines, so this wait costs no second one.
                # They also stand in the running total that phase C reads for its own floors: noted as seen)
                skipped = self.aligner.floor_skipped()[0]
                add_stat(self.stats, "pairs_end_skipped_by_rule", skipped)
                self._floor_seen += skipped
            return start_trim, end_trim
        outs = self._scan_jobs(self._ends_arena(reads), jobs, MODE_TRACE, p.end_size)
        for (side, si), rec in zip(where, outs):
            full, partial = _identities(rec)
            ok = rec[:, 0] != -1
            if si in full_for:
                fulls[(si, side)] = torch.where(ok, full, torch.zeros_like(full))
            rs = rec[:, 0]
            re = rec[:, 1] + 1
            if side == 0:
                cond = ok & (partial > p.end_threshold) & (re != p.end_size) & ((re - rs) >= p.min_trim_size)
                start_trim = torch.where(cond, torch.maximum(start_trim, re + p.extra_end_trim), start_trim)
            else:
                cond = ok & (partial > p.end_threshold) & (rs != 0) & ((re - rs) >= p.min_trim_size)
                end_trim = torch.where(cond, torch.maximum(end_trim, (p.end_size - rs) + p.extra_end_trim), end_trim)
        self.stats["pairs_end"] += sum(int(j[1].shape[0]) for j in jobs)
        return (start_trim, end_trim, fulls) if full_for else (start_trim, end_trim)

    def _hit_paths(self, reads, jobs, sides, hit_first, hits):
        """The paths of the qualifying alignments (Aligner.align_paths, one call): the pair list is built on the device -- a
        hit's read from hit_first, its window and adapter from its job -- and the returned records must carry the hit's
        read_start, read_end, matches, aligned_len and full_len.  -> (heads int32 [H, 4], ops int32 [H, pitch])."""
        if not getattr(self.aligner, "paths", False):
            raise RuntimeError("this aligner returns no alignment paths (Aligner.align_paths)")
        dev = self.device
        H = int(hits.shape[0])
        so, sl = self._end_windows(reads, None, "start")
        eo, el = self._end_windows(reads, None, "end")
        hj = hits[:, 0].to(torch.int64)
        hr = torch.searchsorted(hit_first[1:].contiguous(), torch.arange(H, dtype=torch.int64, device=dev), right=True)
        is_end = torch.tensor([bool(s_) for s_ in sides], dtype=torch.bool, device=dev)[hj]
        off = torch.where(is_end, eo[hr], so[hr]).contiguous()
        length = torch.where(is_end, el[hr], sl[hr]).to(torch.int32).contiguous()
        adapter = torch.tensor([j[0] for j in jobs], dtype=torch.int32, device=dev)[hj].contiguous()
        recs, heads, ops = self.aligner.align_paths(self._ends_arena(reads), off, length, adapter, max_len=self.p.end_size)
        same = (recs[:, 0] == hits[:, 1]) & (recs[:, 1] + 1 == hits[:, 2]) & (recs[:, 5:8] == hits[:, 3:6]).all(dim=1)
        if H and not bool(same.all()):
            k = int(torch.nonzero(~same)[0])
            raise RuntimeError("alignment path of hit %d (read %d, job %d) does not carry the hit's record: %r against %r"
                               % (k, int(hr[k]), int(hj[k]), recs[k].tolist(), hits[k].tolist()))
        return heads, ops

    def phase_b_explain(self, reads: DeviceReads, matching: List[int], bins=None, barcode_threshold: float = 75.0,
                        barcode_diff: float = 5.0, require_two: bool = False, paths: bool = False):
        """Phase B with its reasons kept: -> (start_trim, end_trim int32[R], call -- numpy int64[R] as phase_b_demux gives it,
        or None without bins --, EndExplain).  The trims and the call are the ones phase_b / phase_b_demux return.
        paths=True: the EndExplain also carries the path of every qualifying alignment (_hit_paths; middle hits have none).

        This route runs phase B with EVERY pair traced (prune=False).  Under the exact pruning only the alignments that can
        decide a trim or a call are traced -- the non-deciding alignments and the second-best barcode are deliberately left
        as score records -- so the full lists of qualifying alignments and the second-best scores do not exist there.
        The per-read pass is a library kernel (pc_phase_b_explain); an injected test aligner without it takes the equivalent
        torch formulation, as phase_b does for the trims."""
        R = reads.n
        p = self.p
        dev = self.device
        jobs, where = self._phase_b_jobs(reads, matching)
        J = len(jobs)
        call = None
        if bins is not None:
            job_of = {(si, side): k for k, (side, si) in enumerate(where)}
            jb = [(job_of.get((b[0], 0), -1) if b[0] is not None else -1,
                   job_of.get((b[1], 1), -1) if b[1] is not None else -1) for b in bins]
            call = np.full(R, -1, dtype=np.int64)
        if not jobs or not R:
            summary = torch.zeros((R, 12), dtype=torch.int32, device=dev)
            summary[:, 4:10] = -1
            ex = EndExplain(summary, torch.zeros((R, 4), dtype=torch.float64, device=dev),
                            torch.zeros(R + 1, dtype=torch.int64, device=dev), torch.zeros((0, 6), dtype=torch.int32, device=dev),
                            list(where), bins)
            if paths:
                ex.path_heads = torch.zeros((0, 4), dtype=torch.int32, device=dev)
                ex.path_ops = torch.zeros((0, 1), dtype=torch.int32, device=dev)
            return summary[:, 0].contiguous(), summary[:, 1].contiguous(), call, ex
        sides = [w[0] for w in where]
        outs, out, rec_off = self._scan_jobs(self._ends_arena(reads), jobs, MODE_TRACE, p.end_size, with_layout=True)
        self.stats["pairs_end"] += J * R
        if hasattr(self.aligner, "phase_b_explain"):
            summary, bscore, hit_first, hits = self.aligner.phase_b_explain(
                out, R, rec_off, sides, p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold, bins=jb if bins else None)
            if bins:
                st = torch.zeros(R, dtype=torch.int32, device=dev)
                et = torch.zeros(R, dtype=torch.int32, device=dev)
                c = torch.full((R,), -1, dtype=torch.int32, device=dev)
                self.aligner.phase_b_reduce(out, R, rec_off, sides, p.end_size, p.min_trim_size, p.extra_end_trim, p.end_threshold,
                                            st, et, bins=jb, barcode_threshold=barcode_threshold, barcode_diff=barcode_diff,
                                            require_two=require_two, call=c)
                call = c.to(torch.int64).cpu().numpy()
        else:
            summary, bscore, hit_first, hits, S, E = self._explain_torch(torch.stack(outs), sides, jb if bins else [])
            if bins:
                call = call_barcodes(len(bins), S, E, barcode_threshold, barcode_diff, require_two)
        ex = EndExplain(summary, bscore, hit_first, hits, list(where), bins)
        if paths:
            ex.path_heads, ex.path_ops = self._hit_paths(reads, jobs, sides, hit_first, hits)
        return summary[:, 0].contiguous(), summary[:, 1].contiguous(), call, ex

    def _explain_torch(self, rec, sides, jb):
        """pc_phase_b_explain's contract in torch expressions, for aligners without the kernel (the CPU stand-in of the tests).
        rec [J, R, 8] -> (summary, bscore, hit_first, hits, S, E); S / E float64 [R, K]: the bins' start / end identities,
        NaN where absent (call_barcodes' input)."""
        p = self.p
        dev = self.device
        J, R = int(rec.shape[0]), int(rec.shape[1])
        full, partial = _identities(rec)
        ok = rec[:, :, 0] >= 0                                         # -1 / -2: no alignment
        full = torch.where(ok, full, torch.zeros_like(full))
        rs, re = rec[:, :, 0], rec[:, :, 1] + 1
        is_end = torch.tensor([bool(s) for s in sides], dtype=torch.bool, device=dev)[:, None]
        qual = ok & (partial > p.end_threshold) & ((re - rs) >= p.min_trim_size) & torch.where(is_end, rs != 0, re != p.end_size)
        trim = torch.where(is_end, (p.end_size - rs) + p.extra_end_trim, re + p.extra_end_trim)
        summary = torch.zeros((R, 12), dtype=torch.int32, device=dev)
        for col, side_rows in ((0, ~is_end), (1, is_end)):
            q = qual & side_rows
            t = torch.where(q, trim, torch.zeros_like(trim))
            best = torch.clamp(t.max(dim=0).values, min=0)
            decides = q & (t == best[None, :]) & (best[None, :] > 0)
            summary[:, col] = best
            summary[:, 2 + col] = q.sum(dim=0)
            summary[:, 4 + col] = torch.where(decides.any(dim=0), decides.to(torch.int32).argmax(dim=0), torch.full_like(best, -1))
        # rows: per read, its start alignments in job order, then its end alignments in job order
        order = [j for j, s in enumerate(sides) if s == 0] + [j for j, s in enumerate(sides) if s != 0]
        order_t = torch.tensor(order, dtype=torch.int64, device=dev)
        at = torch.nonzero(qual[order_t].t())                           # (read, position in `order`), row-major
        hr, hj = at[:, 0], order_t[at[:, 1]]
        hits = torch.stack([hj.to(torch.int32), rs[hj, hr], re[hj, hr], rec[hj, hr, 5], rec[hj, hr, 6], rec[hj, hr, 7]], dim=1) \
            if at.shape[0] else torch.zeros((0, 6), dtype=torch.int32, device=dev)
        hit_first = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        hit_first[1:] = torch.cumsum(summary[:, 2].to(torch.int64) + summary[:, 3].to(torch.int64), 0)
        # barcodes: the first two entries of the stable descending sort of each side's present entries
        K = len(jb)
        bscore = torch.zeros((R, 4), dtype=torch.float64, device=dev)
        summary[:, 6:10] = -1
        absent = torch.full((R,), math.nan, dtype=torch.float64, device=dev)
        S = torch.stack([full[b[0]] if b[0] >= 0 else absent for b in jb], dim=1) if K else torch.zeros((R, 0), dtype=torch.float64, device=dev)
        E = torch.stack([full[b[1]] if b[1] >= 0 else absent for b in jb], dim=1) if K else torch.zeros((R, 0), dtype=torch.float64, device=dev)
        for col, x in ((0, S), (1, E)):
            if not K:
                break
            srt = torch.sort(torch.nan_to_num(x, nan=-math.inf), dim=1, descending=True, stable=True)
            for rank in range(min(2, K)):
                present = srt.values[:, rank] > -math.inf
                summary[:, 6 + 2 * col + rank] = torch.where(present, srt.indices[:, rank], torch.full_like(srt.indices[:, rank], -1))
                bscore[:, 2 * col + rank] = torch.where(present, srt.values[:, rank], torch.zeros_like(srt.values[:, rank]))
        return summary, bscore, hit_first, hits, S, E

    # ------------------------------------------------------------------------------------------
    def middle_adapter_list(self, matching: List[int]):
        """porechop.py:541-548: start sequence of every matching set, plus its end sequence when
        that differs from its own start sequence (duplicates across sets are kept, as there)."""
        return [a for a, _ in self._middle_adapters_with_sets(matching)]

    def _middle_adapters_with_sets(self, matching: List[int]):
        """middle_adapter_list with the index of the set each sequence comes from (the pairing hint of _scan_jobs)."""
        ads = []
        for si in matching:
            s = self.sets[si]
            if s.start is not None:
                ads.append((s.start, si))
            if s.end is not None and (s.start is None or s.end[1] != s.start[1]):
                ads.append((s.end, si))
        return ads

    def _prefiltered_scan(self, arena, off, length, max_len, a_list, aidx, hint, ks, ragged, typ_len, packed_reads=None):
        """Whole-read records of the adapters a_list (positions in the middle-adapter list) against the n windows
        (off, length), computed only where the exact prefilter cannot exclude a hit.  SPARSE result
        -> (b [C] int64: position in a_list, w [C] int64: window, rec [C, 8] int32); every (adapter, window) pair that
        is not listed is proven not to be a hit.  The windows that survive for one of a set's sequences are scanned for
        all of that set's sequences in one pass (the set's ahead-of-time kernel)."""
        dev = self.device
        n, B = int(off.shape[0]), len(a_list)
        e64 = torch.empty(0, dtype=torch.int64, device=dev)
        empty = (e64, e64, torch.empty((0, RESULT_INTS), dtype=torch.int32, device=dev))
        if n == 0 or B == 0:
            return empty
        order = None
        pf_off, pf_len = off.contiguous(), length.contiguous()
        if ragged:                                       # a wave runs 64 consecutive windows: similar lengths together
            order = torch.argsort(length, descending=True, stable=True)
            pf_off, pf_len = off[order].contiguous(), length[order].contiguous()
        self.aligner.set_length_hint(typ_len if ragged else 0)
        # packed_reads (reads held at 2 bits per base, `off` in bases): the prefilter scans the PLANE, and only the windows
        # that survive are turned into bytes for the DP; an adapter list the packed route does not take (a letter other than
        # A/C/G/T/U, a piece without seeds) falls back to unpacking everything
        groups, gidx = {}, []
        for a in a_list:
            gidx.append(groups.setdefault(hint[a], len(groups)))
        G = len(groups)
        members = [[b for b in range(B) if gidx[b] == g] for g in range(G)]
        adl, kl = [aidx[a] for a in a_list], [ks[a] for a in a_list]
        packed = packed_reads is not None and packed_reads.arena is None
        if not packed and G <= LEAN_PREFILTER_GROUPS and hasattr(self.aligner, "prefilter_defer_count") \
                and hasattr(torch, "nonzero_static") and not switch_on("PC_NO_LEAN_PREFILTER"):
            scan_off, survivors = off, self._survivors_by_count(arena, pf_off, pf_len, max_len, adl, kl, members, order)
        else:
            arena, scan_off, survivors = self._survivors_by_rows(arena, off, length, pf_off, pf_len, max_len, adl, kl, gidx, G, order,
                                                                 packed_reads if packed else None)
        # per surviving (set, windows): one job per sequence of the set, scanned in one call -> the sparse triple
        cjobs, cmeta = [], []
        for g, sel in survivors:
            so, sl = scan_off[sel], length[sel]
            for b in members[g]:
                cjobs.append((adl[b], so, sl, hint[a_list[b]])); cmeta.append((b, sel))
        if not cjobs:
            return empty
        outs = self._scan_jobs(arena, cjobs, MODE_TWO_PASS, max_len, sort_lengths=ragged, typ_len=typ_len)
        add_stat(self.stats, "pairs_middle_scanned_after_prefilter", sum(int(j[1].shape[0]) for j in cjobs))
        sb = torch.cat([torch.full((int(sel.shape[0]),), b, dtype=torch.int64, device=dev) for b, sel in cmeta])
        return sb, torch.cat([sel for _, sel in cmeta]), torch.cat(outs)

    def _survivors_by_count(self, arena, pf_off, pf_len, max_len, adl, kl, members, order):
        """The windows that survive the prefilter for each adapter set, with ONE host round trip for the whole stage (a handful
        of sets: the usual run).  The library's seed stage leaves its candidate count on the device (pc_prefilter_defer_count),
        the survivors of every set are counted on the device, the counts come back together, and the windows are listed by
        nonzero_static (no further synchronisation).  -> an iterator of (set, windows int64) over the sets with survivors."""
        al, G = self.aligner, len(members)
        glue = choose_glue(al)

        def survivors(defer):
            al.prefilter_defer_count(defer)
            try:
                mask = al.prefilter_mask(arena, pf_off, pf_len, max_len, adl, kl)
            finally:
                al.prefilter_defer_count(False)
            words = int(mask.shape[1])
            gm = []
            for g in range(G):
                for wd in range(words):
                    bits = sum(1 << (b % 32) for b in members[g] if b // 32 == wd)
                    gm.append(bits - (1 << 32) if bits >= (1 << 31) else bits)
            cand, cnt = glue.group_survivors(mask, self._const(gm, torch.int32).view(G, words))
            return cand, cnt.cpu().numpy()                                             # the one synchronisation of this stage
        cand, counts = survivors(True)
        if al.prefilter_overflowed():                    # (rare: the seed list overflowed -- the mask above is incomplete)
            cand, counts = survivors(False)
            add_stat(self.stats, "prefilter_overflow_reruns", 1)
        add_stat(self.stats, "pairs_middle_prefiltered", len(adl) * int(pf_off.shape[0]))
        for g in range(G):
            if counts[g]:
                sel = set_positions(cand[g], int(counts[g]))
                yield g, (sel if order is None else order[sel])

    def _survivors_by_rows(self, arena, off, length, pf_off, pf_len, max_len, adl, kl, gidx, G, order, packed_reads):
        """The same from the prefilter's sparse rows (a barcode panel's many sets, packed-only reads): one compaction over all
        sets.  -> (the arena to scan, the windows' offsets in it, an iterator of (set, windows int64)); packed-only reads
        (packed_reads: the prefilter scans the PLANE, `off` in bases) get an arena of the surviving windows' bytes alone --
        unless the packed route refuses the adapter list, which falls back to unpacking everything."""
        dev, n = self.device, int(off.shape[0])
        got = None
        if packed_reads is not None:
            kw = {"total": True} if self.p.packed_total else {}       # (only then: aligners without the keyword keep working)
            got = self.aligner.prefilter_rows(packed_reads.plane, pf_off, pf_len, max_len, adl, kl, packed=True, **kw)
            if got is None:
                arena = packed_reads.materialize(self.aligner)
                add_stat(self.stats, "packed_route_refused", 1)
        if got is None:
            got = self.aligner.prefilter_rows(arena, pf_off, pf_len, max_len, adl, kl)
        rows, bits = got
        if order is not None:
            rows = order[rows]
        add_stat(self.stats, "pairs_middle_prefiltered", len(adl) * n)
        if G == len(adl):
            cand_g = bits
        else:                                            # union over the sequences of a set
            cand_g = torch.zeros((int(rows.shape[0]), G), dtype=torch.int32, device=dev).index_add_(
                1, self._const(gidx), bits.to(torch.int32)) > 0
        hitg = torch.nonzero(cand_g.t())                              # [C, 2] (group, row), group-major
        scan_off = off
        if packed_reads is not None and packed_reads.arena is None:
            # the surviving windows as bytes, back to back (each padded to 16 bytes + slack), ascending in the plane
            urows = torch.sort(rows).values
            ulen = length[urows].contiguous()
            ustride = (ulen.to(torch.int64) + (8 + 15)) // 16 * 16
            uends = torch.zeros(int(urows.shape[0]) + 1, dtype=torch.int64, device=dev)
            uends[1:] = torch.cumsum(ustride, 0)
            both = torch.cat([torch.bincount(hitg[:, 0], minlength=G), uends[-1:]]).cpu().numpy()   # the one synchronisation of this stage
            counts, utotal = both[:G], int(both[G])
            arena = torch.empty(utotal + 64, dtype=torch.uint8, device=dev)
            arena[utotal:] = ord("N")
            if urows.numel():
                self.aligner.unpack_windows(packed_reads.plane, packed_reads.exc, off[urows].contiguous(), ulen, arena, uends)
            scan_off = torch.full((n,), -1, dtype=torch.int64, device=dev)
            scan_off[urows] = uends[:-1]
            add_stat(self.stats, "bases_unpacked_after_prefilter", utotal)
        else:
            counts = torch.bincount(hitg[:, 0], minlength=G).cpu().numpy()     # the one synchronisation of this stage
        firsts = np.concatenate([[0], np.cumsum(counts)])
        return arena, scan_off, ((g, rows[hitg[int(firsts[g]):int(firsts[g + 1]), 1]]) for g in range(G) if counts[g])

    def phase_c(self, reads: DeviceReads, start_trim, end_trim, matching: List[int], prove: bool = False,
                prefilter: bool = False) -> MiddleHits:
        """nanopore_read.py:210-243 for every read: adapters in order, and for each adapter keep
        re-aligning against the progressively masked read while the hit reaches --middle_threshold.

        Round 0 aligns every adapter against every (unmasked) trimmed read in one go.  That is
        exact for a read up to and including its first hit; only reads with a hit ("dirty", ~1 %)
        get a private masked copy and continue.  Every later round does the same thing for the
        dirty reads still active: ALL adapters against the current masked state, results consumed
        in the reference's order (from the adapter that just hit, which the reference re-aligns)
        up to and including the next hit.  The alignments consumed are exactly the ones the
        reference's nested loops perform, on the same masked sequences; the ones after a hit are
        speculative and discarded.  Rounds = hits of the most-hit read + 1, not alignments.

        prove=True: round 0 runs the score-only pass for every (read, adapter) pair and the
        traceback only for pairs whose score can still mean an identity >= --middle_threshold
        (identity_score_bound) -- everything else is PROVEN not to be a hit, which is all the
        reference does with those alignments.  Hits, masks and splits are identical; the records of
        the proven non-hits are simply not produced.  (An option: it costs a second score pass and a host round
        trip.  The default applies the same bound inside the library instead, between the two passes of its one
        scan -- pc_scan_device_floored: pairs below it are not traced and come back as "no alignment".)

        prefilter=True: the same, with the proof coming from the exact bit-parallel prefilter instead of the
        score pass (pc_prefilter_device: Myers' bit-vector edit distance, one lane per read chunk and adapter; the
        alternative the reference's README.md:355-357 names).  A hit needs full-adapter identity >=
        --middle_threshold, hence at most max_edits(m, threshold) unit-cost edits between the adapter and some
        substring of the read; pairs farther apart are PROVEN not to be hits and never reach the DP.  The reads
        that survive for one of a set's sequences run the two-pass scan for that set (both of its sequences in one
        pass, on the set's ahead-of-time kernel).  Hits, masks, rounds and alignment counts are identical."""
        prove = prove and self.packed_kernels()                # the score bound is derived for the packed kernels' schemes
        ads_sets = self._middle_adapters_with_sets(matching)
        self.middle_adapters = [a for a, _ in ads_sets]
        if not ads_sets or reads.n == 0:
            return MiddleHits.none(self.device)
        return MiddleScan(self, reads, ads_sets, prove, prefilter).run(start_trim, end_trim)

    def middle_hit_paths(self, reads: DeviceReads, start_trim, end_trim, hits: MiddleHits):
        """The alignment path of every middle hit of phase_c (same reads, trims and matching sets; hits.adapter indexes the
        middle adapters of that call) -> (records int32 [H, 8], heads int32 [H, 4], ops int32 [H, pitch]) in trimmed-read
        coordinates, row for row with `hits` (Aligner.middle_paths, one call).  The masked read of a later round is rebuilt
        from the hit list (middle_mask_tables) and only a bounded window around the hit is aligned.
        Every returned record must carry its hit's read_start, read_end and full identity: a difference raises."""
        al = self.aligner
        if not getattr(al, "middle_paths", False):
            raise RuntimeError("this aligner returns no paths for middle hits (Aligner.middle_paths)")
        dev = self.device
        H = int(hits.read.shape[0])
        if H == 0:
            return (torch.zeros((0, RESULT_INTS), dtype=torch.int32, device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev),
                    torch.zeros((0, 1), dtype=torch.int32, device=dev))
        if reads.arena is None:
            reads.materialize(al)                                    # every base of a window is needed as a byte
        glue = choose_glue(al)
        toff, tlen, _ = glue.trim_windows(reads.off, reads.length, start_trim, end_trim)
        aidx = torch.tensor([self.seq_index[a[1]] for a in self.middle_adapters], dtype=torch.int32, device=dev)
        intervals, mask_base, mask_count = middle_mask_tables(hits.read, hits.start, hits.end)
        read_off = toff[hits.read].to(torch.int64).contiguous()
        read_len = tlen[hits.read].to(torch.int32).contiguous()
        recs, heads, ops = al.middle_paths(reads.arena, read_off, read_len, aidx[hits.adapter.to(torch.int64)].contiguous(),
                                           hits.end.to(torch.int32).contiguous(), mask_base, mask_count, intervals)
        # (the %f-rounded full identity, from the code phase_c got the hits' from)
        full = glue.middle_hits(recs, self.p.middle_threshold)[0]
        same = (recs[:, 0] == hits.start) & (recs[:, 1] + 1 == hits.end) & (full == hits.identity)
        if not bool(same.all()):
            k = int(torch.nonzero(~same)[0])
            raise RuntimeError("alignment path of middle hit %d (read %d, adapter %d, %d-%d, identity %r) carries another record: %r"
                               % (k, int(hits.read[k]), int(hits.adapter[k]), int(hits.start[k]), int(hits.end[k]),
                                  float(hits.identity[k]), recs[k].tolist()))
        return recs, heads, ops

    def close(self):
        self.aligner.close()
