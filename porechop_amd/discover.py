"""`python -m porechop_amd.discover -i reads.fastq` -- what is on the ends of these reads?

The package trims what panel.json lists.  A run whose adapters are not in that table (a newer kit, a custom primer) finds
no set in phase A and leaves every read untrimmed.  This module answers the question from the reads themselves:

  census      every k-mer of every read's first and last end_size bases, counted on the GPU into one dense table per
              side (Aligner.kmer_count, csrc/pc_discover.hip) -- all reads, not a sample
  candidates  the table entries seen in at least min_fraction of the windows (Aligner.kmer_candidates)
  assembly    assemble(): greedy walks through the candidates' de Bruijn graph, from the most frequent k-mer outwards,
              as long as the next k-mer keeps extend_ratio of the seed's count -- an adapter is a path of k-mers of about
              equal count, and a k-mer that holds one base of the read behind it has about a quarter of that
  annotation  every assembled sequence against every sequence of the panel (one Aligner.align_pairs call): the nearest
              known adapter and its full identity; at adapter_threshold or above the sequence is `known`
  use         Discovery.adapter_sets() -> AdapterSet list for runner.run(adapter_panel=load_panel() + ...); the FASTA
              form (write_adapters / read_adapters) carries such sets from one run to the next

  barcodes    discover(barcodes=True) / --barcodes: every found sequence is an anchor; the L bases right behind (start) or
              before (end) its alignment in every window (Aligner.anchor_inserts over one scan per block) are counted as
              whole inserts, cluster_inserts() merges error and shift shadows into the most frequent insert they resemble,
              pair_barcodes() joins start and end barcodes; Discovery.barcode_sets() -> barcode sets for a -b DIR run

assemble(), cluster_inserts(), pair_barcodes() and the FASTA functions are plain Python and numpy: they load neither torch
nor the library.
DESIGN.md section 13 has the contract, the tie rules and the costs."""
import math
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

BASES = "ACGT"


@dataclass
class Found:
    sequence: str
    peak: int                          # count of the seed k-mer
    support: int                       # lowest count of a k-mer on the path
    nearest: Optional[str] = None      # annotation (discover): name of the nearest panel sequence,
    identity: float = 0.0              # its full identity in percent,
    known: bool = False                # and whether that reaches adapter_threshold
    alignment: Optional[str] = None    # discover(alignments=True): render_alignment of the sequence (as the read) against it


def min_count(n_windows, min_fraction=0.05):
    """The count a k-mer needs to be a candidate: max(2, ceil(min_fraction * n_windows))."""
    return max(2, int(math.ceil(min_fraction * n_windows)))


def decode(code, k):
    """k-mer code (2 bits per base, first base in the highest bits, A C G T = 0 1 2 3) -> string."""
    return "".join(BASES[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def assemble(codes, counts, k, n_windows, min_fraction=0.05, extend_ratio=0.5, min_len=None) -> List[Found]:
    """k-mer counts of n_windows windows -> the sequences they spell, in discovery order.

    1. candidates: count >= min_count(n_windows, min_fraction)
    2. seed: the unused candidate with the highest count (ties: the lowest code)
    3. extend right: of the four successors ((cur << 2) & mask) | b take the unused candidate with the highest count (ties:
       the lowest b) if it has at least extend_ratio x the SEED's count; mark it used; repeat from it
    4. extend left from the seed the same way (predecessors (cur >> 2) | (b << 2 (k - 1)))
    5. emit Found(sequence, peak = seed count, support = lowest count on the path); back to 2
    6. drop sequences shorter than min_len (default k + 4)
    Every k-mer is used once, so every cycle ends (a homopolymer's k-mer is its own successor: used, not taken)."""
    k = int(k)
    if min_len is None:
        min_len = k + 4
    codes = np.asarray(codes, dtype=np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    keep = counts >= min_count(n_windows, min_fraction)
    codes, counts = codes[keep], counts[keep]
    order = np.lexsort((codes, -counts))
    table = dict(zip(codes.tolist(), counts.tolist()))
    used = set()
    mask = (1 << (2 * k)) - 1
    top = 2 * (k - 1)
    out = []

    def walk(cur, floor, step):
        """-> ([base, ...], [count, ...]) of the k-mers taken from `cur` outwards"""
        bases, seen = [], []
        while True:
            best, best_count, best_b = None, -1, -1
            for b in range(4):
                nxt = step(cur, b)
                c = table.get(nxt)
                if c is not None and nxt not in used and c > best_count:
                    best, best_count, best_b = nxt, c, b
            if best is None or best_count < floor:
                return bases, seen
            used.add(best)
            bases.append(best_b)
            seen.append(best_count)
            cur = best

    for seed in codes[order].tolist():
        if seed in used:
            continue
        used.add(seed)
        peak = table[seed]
        floor = extend_ratio * peak
        right, rc = walk(seed, floor, lambda cur, b: ((cur << 2) & mask) | b)
        left, lc = walk(seed, floor, lambda cur, b: (cur >> 2) | (b << top))
        seq = "".join(BASES[b] for b in reversed(left)) + decode(seed, k) + "".join(BASES[b] for b in right)
        if len(seq) >= min_len:
            out.append(Found(seq, int(peak), int(min([peak] + rc + lc))))
    return out


# ---- barcodes: whole inserts behind a found sequence ---------------------------------------------------------------------
@dataclass
class BarcodeFound:
    sequence: str
    peak: int                          # windows whose insert is exactly this sequence
    support: int                       # peak + the counts of the shadows merged into it
    partner: Optional[int] = None      # pair_barcodes: index of the centroid on the other side that belongs to the same barcode
    nearest: Optional[str] = None      # annotation, as for Found
    identity: float = 0.0
    known: bool = False


@dataclass
class AnchorInserts:
    """What lies behind one found sequence (the anchor) of one side."""
    anchor: int                        # index into Discovery.start / Discovery.end
    anchored: int = 0                  # windows that gave an insert
    barcodes: List[BarcodeFound] = field(default_factory=list)      # the centroids, when there are at least two
    constant: Optional[BarcodeFound] = None                         # a single centroid: the adapter simply goes on; no barcode
    sequence: Optional[str] = None     # the anchor as it was scanned: the found sequence, its inner edge trimmed (trim_anchor)


def trim_anchor(sequence, side, count_of, k, edge_ratio=0.9):
    """A found sequence as the anchor of the barcode pass: its inner edge -- the right end on the start side (0), the left end on
    the end side (1) -- taken back while the edge base is not common to the reads that carry the bases before it.

    assemble() lets a sequence grow while the next k-mer keeps extend_ratio (0.5) of the SEED's count, so a first barcode base
    that half of the barcodes share is taken into the adapter, and every insert behind such an anchor begins one base late.
    The census tells the two apart: inside an adapter the edge k-mer and the k-mer one step inward need the same k - 1 bases
    and one more each, so their counts are about equal whatever the error rate; where the edge base is a barcode's, shared by
    a share p of the reads, the edge k-mer has about p times the inward one's count.  The edge base is dropped while
    count_of(edge k-mer) < edge_ratio * count_of(inward k-mer); count_of: k-mer code -> its count in the side's table.
    -> the anchor (at least k bases of the sequence)."""
    seq = sequence
    while len(seq) > k:
        edge, inward = (seq[-k:], seq[-k - 1:-1]) if side == 0 else (seq[:k], seq[1:k + 1])
        if count_of(_encode(edge)) >= edge_ratio * count_of(_encode(inward)):
            break
        seq = seq[:-1] if side == 0 else seq[1:]
    return seq


def reverse_complement(seq):
    return seq[::-1].translate(str.maketrans("ACGT", "TGCA"))


def edit_distance(a, b):
    """Unit-cost edit distance of two strings."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def shift_distance(a, b, max_shift=4):
    """sd(a, b) = min over s = 0..max_shift of min(ed(a[s:], b[:L-s]), ed(b[s:], a[:L-s])), L = len(a) = len(b): the edit
    distance of two inserts of which one may have been cut up to max_shift bases later than the other."""
    L = len(a)
    assert len(b) == L
    return min(min(edit_distance(a[s:], b[:L - s]), edit_distance(b[s:], a[:L - s])) for s in range(min(max_shift, L - 1) + 1))


def _ed_rows(a, b):
    """edit_distance for m pairs at once: a int[m, p], b int[m, q] -> int64[m] (row by row; the dependency along a row --
    cur[j] = min(cur[j], cur[j-1] + 1) -- is a running minimum of cur[j] - j)."""
    m, q = b.shape
    ramp = np.arange(q + 1, dtype=np.int64)
    prev = np.broadcast_to(ramp, (m, q + 1)).copy()
    for i in range(a.shape[1]):
        cur = np.empty_like(prev)
        cur[:, 0] = i + 1
        np.minimum(prev[:, :-1] + (a[:, i:i + 1] != b), prev[:, 1:] + 1, out=cur[:, 1:])
        prev = np.minimum.accumulate(cur - ramp, axis=1) + ramp
    return prev[:, -1]


def _sd_to_all(x, centroids, max_shift):
    """shift_distance of x int[L] to every row of centroids int[c, L] -> int64[c]"""
    c, L = centroids.shape
    xs = np.broadcast_to(x, (c, L))
    best = np.full(c, L, dtype=np.int64)
    for s in range(min(max_shift, L - 1) + 1):
        best = np.minimum(best, _ed_rows(xs[:, s:], centroids[:, :L - s]))
        best = np.minimum(best, _ed_rows(centroids[:, s:], xs[:, :L - s]))
    return best


def insert_floor(n_anchored, min_share=0.001, min_count=3):
    """The count an exact insert needs to be a candidate: max(min_count, ceil(min_share * n_anchored))."""
    return max(int(min_count), int(math.ceil(min_share * n_anchored)))


def cluster_inserts(codes, counts, L, n_anchored, min_share=0.001, min_count=3, min_dist=5, max_shift=4) -> List[BarcodeFound]:
    """Exact insert counts of one anchor (codes as Aligner.anchor_inserts returns them, L bases each) -> the centroids.

    1. candidates: count >= insert_floor(n_anchored, min_share, min_count); sorted by count descending, then code ascending
    2. in that order: a candidate whose shift_distance to some accepted centroid is below min_dist is a shadow -- an error or
       shift copy -- and its count goes to the `support` of the FIRST such centroid; any other candidate becomes a centroid
    3. -> the centroids in that order: sequence, peak (own exact count), support
    Fewer than two centroids are no barcodes (a single one is the adapter's constant continuation): the caller decides."""
    L = int(L)
    codes = np.asarray(codes, dtype=np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    keep = counts >= insert_floor(n_anchored, min_share, min_count)
    codes, counts = codes[keep], counts[keep]
    order = np.lexsort((codes, -counts))
    codes, counts = codes[order], counts[order]
    shifts = 2 * (L - 1 - np.arange(L, dtype=np.int64))
    digits = (codes[:, None] >> shifts[None, :]) & 3                # [candidates, L] base codes
    out, rows = [], np.zeros((0, L), dtype=np.int64)
    for x, code, count in zip(digits, codes.tolist(), counts.tolist()):
        if out:
            near = np.nonzero(_sd_to_all(x, rows, max_shift) < min_dist)[0]
            if near.size:
                out[int(near[0])].support += int(count)
                continue
        out.append(BarcodeFound(decode(code, L), int(count), int(count)))
        rows = np.concatenate([rows, x[None, :]])
    return out


def pair_barcodes(start: List[BarcodeFound], end: List[BarcodeFound], start_codes=None, end_codes=None):
    """Which start centroid and which end centroid are one barcode -> [(i, j)], and the `partner` fields set.

    1. start centroid i pairs with the end centroid whose sequence is its reverse complement, if there is one
    2. the rest by co-occurrence: start_codes / end_codes hold one insert code per read (the same reads, the same order;
       negative: none); count the reads whose two inserts EQUAL centroids i and j exactly; i and j pair when each is the
       other's best partner with a count of at least 2 (ties: the lowest index)
    3. anything else stays one-sided (partner None)"""
    for f in start + end:
        f.partner = None
    pairs = []
    where = {}
    for j, f in enumerate(end):
        where.setdefault(f.sequence, j)
    for i, f in enumerate(start):
        j = where.get(reverse_complement(f.sequence))
        if j is not None and end[j].partner is None:
            f.partner, end[j].partner = j, i
            pairs.append((i, j))
    left_i = [i for i, f in enumerate(start) if f.partner is None]
    left_j = [j for j, f in enumerate(end) if f.partner is None]
    if left_i and left_j and start_codes is not None and end_codes is not None:
        sc = np.asarray(start_codes, dtype=np.int64).reshape(-1)
        ec = np.asarray(end_codes, dtype=np.int64).reshape(-1)
        assert sc.shape == ec.shape
        row = {_encode(start[i].sequence): a for a, i in enumerate(left_i)}
        col = {_encode(end[j].sequence): b for b, j in enumerate(left_j)}
        table = np.zeros((len(left_i), len(left_j)), dtype=np.int64)
        both = (sc >= 0) & (ec >= 0)
        for s, e in zip(sc[both].tolist(), ec[both].tolist()):
            a, b = row.get(s), col.get(e)
            if a is not None and b is not None:
                table[a, b] += 1
        best_of_row = table.argmax(axis=1)                           # (argmax: the first, i.e. lowest index, of equals)
        best_of_col = table.argmax(axis=0)
        for a, i in enumerate(left_i):
            b = int(best_of_row[a])
            if table[a, b] >= 2 and int(best_of_col[b]) == a:
                start[i].partner, end[left_j[b]].partner = left_j[b], i
                pairs.append((i, left_j[b]))
    return sorted(pairs)


def _encode(seq):
    v = 0
    for ch in seq:
        v = (v << 2) | BASES.index(ch)
    return v


@dataclass
class Discovery:
    start: List[Found] = field(default_factory=list)
    end: List[Found] = field(default_factory=list)
    reads: int = 0                     # reads counted
    windows: int = 0                   # windows counted: one start and one end window per read
    k: int = 12
    # discover(barcodes=True): per side ("start", "end"), one AnchorInserts per found sequence of that side
    barcodes: dict = field(default_factory=dict)

    def barcode_anchor(self, side):
        """The first anchor of `side` ("start" / "end") with barcodes -- the one pair_barcodes was run on -- or None."""
        return next((a for a in self.barcodes.get(side, []) if a.barcodes), None)

    def barcode_sets(self, prefix="discovered"):
        """The barcodes that are NOT known, as barcode sets for runner.run(adapter_panel=..., barcode_dir=...): centroid i
        (from 1, in the start side's order) of the first start anchor with barcodes gives
        AdapterSet("Barcode <prefix>_i (forward)", ("<set name>_start", sequence), ("<set name>_end", its partner's sequence)),
        one-sided where it has no partner.  The names pass panel.is_barcode and choose_barcoding_kit, survive write_adapters /
        read_adapters unchanged, and the bin is panel.barcode_name's.  Only sets with a start sequence are emitted
        (panel.barcode_direction reads start[0]): centroids seen on the end side alone are reported, not emitted."""
        from .pipeline import AdapterSet
        s, e = self.barcode_anchor("start"), self.barcode_anchor("end")
        sets = []
        for i, f in enumerate(s.barcodes if s is not None else []):
            if f.known:
                continue
            name = "Barcode %s_%d (forward)" % (prefix, i + 1)
            other = e.barcodes[f.partner] if e is not None and f.partner is not None else None
            sets.append(AdapterSet(name, (name + "_start", f.sequence),
                                   (name + "_end", other.sequence) if other is not None and not other.known else None))
        return sets

    def adapter_sets(self, prefix="discovered"):
        """The sequences that are NOT known, as adapter sets for runner.run(adapter_panel=...): new start sequence i and new
        end sequence i (discovery order, from 1) make AdapterSet("<prefix>_i", ("<prefix>_i_start", seq), ("<prefix>_i_end",
        seq)); a side without a partner gives a one-sided set."""
        from .pipeline import AdapterSet
        starts = [f.sequence for f in self.start if not f.known]
        ends = [f.sequence for f in self.end if not f.known]
        sets = []
        for i in range(max(len(starts), len(ends))):
            name = "%s_%d" % (prefix, i + 1)
            sets.append(AdapterSet(name, (name + "_start", starts[i]) if i < len(starts) else None,
                                   (name + "_end", ends[i]) if i < len(ends) else None))
        return sets


# ---- FASTA of adapter sets ---------------------------------------------------------------------------------------------
def write_adapters(path, sets):
    """One record per sequence: ><set name>_start / ><set name>_end.  -> path"""
    with open(path, "w") as fh:
        for s in sets:
            for suffix, side in (("_start", s.start), ("_end", s.end)):
                if side is not None:
                    fh.write(">%s%s\n%s\n" % (s.name, suffix, side[1]))
    return path


def read_adapters(path):
    """The sets write_adapters wrote (records of one set need not be adjacent; sets come in order of first appearance).  A
    record whose name ends in neither _start nor _end is refused."""
    from .pipeline import AdapterSet
    records, name = [], None
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                name = line[1:].strip()
                records.append([name, ""])
            elif name is None:
                raise ValueError("Error: %s does not begin with a FASTA header" % path)
            else:
                records[-1][1] += line.upper()
    sets = {}
    for name, seq in records:
        for suffix in ("_start", "_end"):
            if name.endswith(suffix) and len(name) > len(suffix):
                s = sets.setdefault(name[:-len(suffix)], AdapterSet(name[:-len(suffix)]))
                if getattr(s, suffix[1:]) is not None:
                    raise ValueError("Error: adapter record %r appears twice in %s" % (name, path))
                if not seq:
                    raise ValueError("Error: adapter record %r in %s has no sequence" % (name, path))
                setattr(s, suffix[1:], (name, seq))
                break
        else:
            raise ValueError("Error: adapter record %r in %s must be named <set>_start or <set>_end" % (name, path))
    return list(sets.values())


# ---- the census ----------------------------------------------------------------------------------------------------------
def end_windows(off, length, end_size):
    """The windows phase B scans (Pipeline._end_windows; nanopore_read.py:155,160): start [0, min(L, end_size)), end
    [max(0, L - end_size), L) -> (start offsets, end offsets, window lengths)."""
    import torch
    wl = torch.clamp(length, max=int(end_size))
    return off, off + (length - wl).to(torch.int64), wl.contiguous()


def _blocks(input_path):
    """The reads as runner.run takes them: a file above the streaming limit block by block with run_streamed's loaders (all
    blocks of a file that turns out not to be streamable: one whole load), anything else whole."""
    from . import runner
    from .io import GzStream, ReadSet
    block = runner._stream_block_bytes()
    if os.path.isfile(input_path) and os.path.getsize(input_path) * (3 if runner._is_gzip(input_path) else 1) > 2 * block:
        if runner._is_gzip(input_path):
            gz = GzStream(input_path)
            try:
                rs = gz.next(block)
                if rs:
                    while rs:
                        yield rs
                        rs = gz.next(block)
                    if rs is False:
                        raise ValueError("Error: " + input_path + " could not be parsed - is it formatted correctly?")
                    return
            finally:
                gz.close()
        else:
            size, pos = os.path.getsize(input_path), 0
            rs, nxt = ReadSet.segment(input_path, 0, block)
            if rs is not None:
                while True:
                    yield rs
                    pos = nxt
                    if pos >= size:
                        return
                    rs, nxt = ReadSet.segment(input_path, pos, block)
                    if rs is None or nxt <= pos:
                        raise ValueError("Error: " + input_path + " could not be parsed - is it formatted correctly?")
    yield runner._load(input_path, 0)[0]


def _barcode_pass(aligner, input_path, found, end_size, max_reads, dev, barcode_len, anchor_identity, cluster_options):
    """The second pass of discover(barcodes=True): every found sequence of a side is an anchor (found: the two sides' anchor
    strings, trim_anchor of the found sequences, in their order).  Per block of reads, one scan
    of the start windows against every start anchor and of the end windows against every end anchor (one job per anchor),
    Aligner.anchor_inserts per anchor, and the block's exact insert counts (torch.unique) added to a host counter per (side,
    anchor).  -> {"start": [AnchorInserts], "end": [AnchorInserts]}, the first anchor with barcodes of either side paired
    with the other's (pair_barcodes).  Replaces the aligner's adapter table by the anchors."""
    import torch
    from . import runner
    from .batch import RESULT_INTS
    anchors = [(side, a, seq) for side in range(2) for a, seq in enumerate(found[side])]
    result = {name: [AnchorInserts(a, sequence=seq) for a, seq in enumerate(found[side])] for side, name in enumerate(("start", "end"))}
    if not anchors:
        return result
    aligner.set_adapters([seq for _, _, seq in anchors])
    tables = [{} for _ in anchors]                                  # insert code -> count
    per_read = [[] for _ in anchors]                                # one int64 array of codes per block
    n = 0
    for rs in _blocks(str(input_path)):
        try:
            hi = rs.count if max_reads is None else min(rs.count, int(max_reads) - n)
            reads = runner._upload(rs, dev, 0, hi)
            if reads is not None:
                s_off, e_off, wl = end_windows(reads.off, reads.length, end_size)
                offs = [s_off.contiguous(), e_off.contiguous()]
                woff = torch.cat([offs[side] for side, _, _ in anchors])
                wlen = torch.cat([wl] * len(anchors))
                out = torch.empty((hi * len(anchors), RESULT_INTS), dtype=torch.int32, device=woff.device)
                aligner.scan_device(reads.arena, woff, wlen, np.arange(len(anchors), dtype=np.int32),
                                    hi * np.arange(len(anchors) + 1, dtype=np.int64), end_size, out)
                for j, (side, _, seq) in enumerate(anchors):
                    codes = aligner.anchor_inserts(reads.arena, offs[side], wl, out[j * hi:(j + 1) * hi], len(seq), side,
                                                   min_identity=anchor_identity, insert_len=barcode_len)
                    values, counts = torch.unique(codes[codes >= 0], return_counts=True)
                    for v, c in zip(values.tolist(), counts.tolist()):
                        tables[j][v] = tables[j].get(v, 0) + c
                    per_read[j].append(codes.cpu().numpy())
                n += hi
        finally:
            rs.close()
        if max_reads is not None and n >= int(max_reads):
            break
    for j, (side, a, _) in enumerate(anchors):
        item = result[("start", "end")[side]][a]
        item.anchored = int(sum(tables[j].values()))
        centroids = cluster_inserts(list(tables[j].keys()), list(tables[j].values()), barcode_len, item.anchored, **cluster_options)
        if len(centroids) >= 2:
            item.barcodes = centroids
        elif centroids:
            item.constant = centroids[0]
    first = [next((j for j, (side, a, _) in enumerate(anchors) if side == want and result[("start", "end")[side]][a].barcodes), None)
             for want in range(2)]
    if first[0] is not None and first[1] is not None:
        pair_barcodes(result["start"][anchors[first[0]][1]].barcodes, result["end"][anchors[first[1]][1]].barcodes,
                      np.concatenate(per_read[first[0]]), np.concatenate(per_read[first[1]]))
    return result


def discover(input_path, k=12, end_size=150, max_reads=None, device=None, aligner=None, adapter_threshold=90.0,
             alignments=False, barcodes=False, barcode_len=24, anchor_identity=75, barcode_min_share=0.001, barcode_min_count=3,
             barcode_min_dist=5, anchor_edge_ratio=0.9, **assemble_options) -> Discovery:
    """Census, assembly and annotation of one input (file or Albacore directory) -> Discovery.
    max_reads: count only the first so many reads.  aligner: an Aligner of `device` to use (its adapter table is replaced by
    the panel's sequences); default: one of its own.  alignments: every found sequence also gets the alignment against its
    nearest known adapter, drawn (Found.alignment; Aligner.align_pairs_paths).  assemble_options: min_fraction, extend_ratio,
    min_len.
    barcodes: a second pass over the same reads looks for barcodes behind every found sequence (Discovery.barcodes,
    Discovery.barcode_sets): inserts of barcode_len bases (1..31) next to alignments of at least anchor_identity percent (an
    integer, 0..100), clustered by cluster_inserts(min_share=barcode_min_share, min_count=barcode_min_count,
    min_dist=barcode_min_dist).  An anchor is the found sequence with its inner edge trimmed by trim_anchor(edge_ratio=
    anchor_edge_ratio); Discovery.start / end are what they are without the option."""
    import torch
    from . import runner
    from .batch import Aligner, records_to_fields
    from .panel import load_panel
    k, end_size = int(k), int(end_size)
    if not 4 <= k <= 13:
        raise ValueError("Error: k must be between 4 and 13")
    if barcodes:
        barcode_len, anchor_identity = int(barcode_len), int(anchor_identity)
        if not 1 <= barcode_len <= 31:                 # (at 32 a code fills the sign bit: pc_anchor_inserts)
            raise ValueError("Error: barcode_len must be between 1 and 31")
        if not 0 <= anchor_identity <= 100:
            raise ValueError("Error: anchor_identity must be between 0 and 100")
    names, seqs = [], []                               # the panel's distinct sequences, each under its first name
    for s in load_panel():
        for side in (s.start, s.end):
            if side is not None and side[1] not in seqs:
                names.append(side[0])
                seqs.append(side[1])
    dev = torch.device(device if device is not None else ("cuda" if aligner is None else "cpu"))
    own = aligner is None
    if own:
        aligner = Aligner(seqs, device=dev.index if dev.index is not None else torch.cuda.current_device())
    else:
        aligner.set_adapters(seqs)
    try:
        tables, n = None, 0
        import contextlib
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            for rs in _blocks(str(input_path)):
                try:
                    hi = rs.count if max_reads is None else min(rs.count, int(max_reads) - n)
                    reads = runner._upload(rs, dev, 0, hi)
                    if reads is not None:
                        if tables is None:
                            tables = [torch.zeros(1 << (2 * k), dtype=torch.int32, device=dev) for _ in range(2)]
                        s_off, e_off, wl = end_windows(reads.off, reads.length, end_size)
                        aligner.kmer_count(reads.arena, s_off.contiguous(), wl, k, counts=tables[0])
                        aligner.kmer_count(reads.arena, e_off.contiguous(), wl, k, counts=tables[1])
                        n += hi
                finally:
                    rs.close()
                if max_reads is not None and n >= int(max_reads):
                    break
            found = [[], []]
            if tables is not None:
                floor = min_count(n, assemble_options.get("min_fraction", 0.05))
                for side in range(2):
                    codes, counts = aligner.kmer_candidates(tables[side], k, floor)
                    found[side] = assemble(codes, counts, k, n, **assemble_options)
            inserts = {}
            if barcodes:
                trimmed = [[trim_anchor(f.sequence, side, lambda code, t=tables[side]: int(t[code]), k, anchor_edge_ratio)
                            for f in found[side]] for side in range(2)]
                inserts = _barcode_pass(aligner, input_path, trimmed, end_size, max_reads, dev, barcode_len, anchor_identity,
                                        dict(min_share=barcode_min_share, min_count=barcode_min_count, min_dist=barcode_min_dist))
                aligner.set_adapters(seqs)                         # (the pass scanned with the anchors as its adapter table)
        every = found[0] + found[1] + [b for side in ("start", "end") for a in inserts.get(side, [])
                                       for b in a.barcodes + ([a.constant] if a.constant is not None else [])]
        if every:
            rec = aligner.align_pairs([(f.sequence, a) for f in every for a in range(len(seqs))])
            full = records_to_fields(rec)[0].reshape(len(every), len(seqs))
            bests = []
            for f, row in zip(every, full):
                best = int(np.argmax(row))                         # (the first of equals: panel order)
                f.nearest, f.identity = names[best], float(row[best])
                f.known = f.identity >= adapter_threshold
                bests.append(best)
            if alignments:
                from .batch import render_alignment
                if not getattr(aligner, "paths", False):
                    raise RuntimeError("this aligner returns no alignment paths (Aligner.align_pairs_paths)")
                drawn = found[0] + found[1]                        # (the found sequences: `every` begins with them)
                _, heads, strings = aligner.align_pairs_paths(list(zip([f.sequence for f in drawn], bests)))
                for f, best, head, text in zip(drawn, bests, heads, strings):
                    f.alignment = render_alignment(f.sequence, seqs[best], head, text)
        return Discovery(found[0], found[1], reads=n, windows=2 * n, k=k, barcodes=inserts)
    finally:
        if own:
            aligner.close()


# ---- command line --------------------------------------------------------------------------------------------------------
def report_lines(d: Discovery, alignments=False):
    """One line per found sequence: side, sequence, peak, support, share of the side's windows, nearest known adapter, its
    identity, known / new.  alignments: under each line the three lines of its alignment against that adapter (the found
    sequence above, the adapter below, '|' between equal bases, '-' for gaps), indented by two blanks."""
    lines = []
    for side, found in (("start", d.start), ("end", d.end)):
        for f in found:
            lines.append("%s\t%s\t%d\t%d\t%.4f\t%s\t%.1f\t%s" % (side, f.sequence, f.peak, f.support, f.peak / max(1, d.reads),
                                                               f.nearest, f.identity, "known" if f.known else "new"))
            if alignments and f.alignment is not None:
                lines += ["  " + row for row in f.alignment.split("\n")]
    return lines


def barcode_report_lines(d: Discovery):
    """One line per barcode of discover(barcodes=True): side, anchor (index of the found sequence of that side it lies
    behind), sequence, peak, support, share of the anchor's anchored windows, partner (index of the other side's centroid, or
    -), known / new.  An anchor's single centroid is no barcode: its line ends in `constant`."""
    lines = []
    for side in ("start", "end"):
        for a in d.barcodes.get(side, []):
            for f, status in [(f, "known" if f.known else "new") for f in a.barcodes] + ([(a.constant, "constant")] if a.constant else []):
                lines.append("%s\t%d\t%s\t%d\t%d\t%.4f\t%s\t%s" % (side, a.anchor, f.sequence, f.peak, f.support,
                                                                 f.support / max(1, a.anchored),
                                                                 "-" if f.partner is None else str(f.partner), status))
    return lines


def main(argv=None):
    from .__main__ import build_parser, run_cli
    p = build_parser(prog="porechop_amd.discover")
    p.add_argument("--k", type=int, default=12, help="k-mer length of the census (4..13)")
    p.add_argument("--min_fraction", type=float, default=0.05, help="a candidate k-mer occurs in at least this share of the windows")
    p.add_argument("--extend_ratio", type=float, default=0.5, help="a sequence grows while the next k-mer keeps this share of its seed's count")
    p.add_argument("--min_len", type=int, default=None, help="shortest sequence reported (default: k + 4)")
    p.add_argument("--max_reads", type=int, default=None, help="count only the first so many reads (default: all)")
    p.add_argument("--adapters_out", help="write the new sequences as a FASTA of adapter sets")
    p.add_argument("--extra_adapters", help="FASTA of adapter sets (as --adapters_out writes it) to add to the panel of the run")
    p.add_argument("--alignments", action="store_true",
                   help="under every found sequence, draw its alignment against the nearest known adapter")
    p.add_argument("--barcodes", action="store_true", help="look for barcodes behind every found sequence (a second pass over the reads)")
    p.add_argument("--barcode_len", type=int, default=24, help="bases taken next to a found sequence (1..31)")
    p.add_argument("--anchor_identity", type=int, default=75,
                   help="a found sequence's alignment counts with at least this full identity in percent (an integer)")
    p.add_argument("--barcode_min_share", type=float, default=0.001, help="an exact insert is a candidate in at least this share of the anchored windows")
    p.add_argument("--barcode_min_count", type=int, default=3, help="... and at least this often")
    p.add_argument("--barcode_min_dist", type=int, default=5, help="a candidate nearer than this to a more frequent barcode is merged into it")
    p.add_argument("--anchor_edge_ratio", type=float, default=0.9,
                   help="a found sequence's innermost base is kept as part of the anchor while its k-mer has this share of the count of the k-mer before it")
    a = p.parse_args(argv)
    try:
        extra = read_adapters(a.extra_adapters) if a.extra_adapters else []
        bc = dict(barcodes=True, barcode_len=a.barcode_len, anchor_identity=a.anchor_identity, barcode_min_share=a.barcode_min_share,
                  barcode_min_count=a.barcode_min_count, barcode_min_dist=a.barcode_min_dist,
                  anchor_edge_ratio=a.anchor_edge_ratio) if a.barcodes else {}
        d = discover(a.input, k=a.k, end_size=a.end_size, max_reads=a.max_reads, adapter_threshold=a.adapter_threshold,
                     min_fraction=a.min_fraction, extend_ratio=a.extend_ratio, min_len=a.min_len, alignments=a.alignments, **bc)
    except ValueError as e:
        sys.exit(str(e))
    except RuntimeError as e:
        sys.exit("Error: " + str(e))
    print("\n".join(["side\tsequence\tpeak\tsupport\tshare\tnearest\tidentity\tstatus"] + report_lines(d, a.alignments)))
    new = d.adapter_sets()
    if a.barcodes:
        print("\n".join(["side\tanchor\tbarcode\tpeak\tsupport\tshare\tpartner\tstatus"] + barcode_report_lines(d)))
        new = new + d.barcode_sets()
    if a.adapters_out:
        write_adapters(a.adapters_out, new)
    if a.output is not None or a.barcode_dir is not None:
        from .panel import load_panel
        run_cli(a, adapter_panel=load_panel() + new + extra)


if __name__ == "__main__":
    main()
