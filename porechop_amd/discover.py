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

assemble() and the FASTA functions are plain Python and numpy: they load neither torch nor the library.
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


@dataclass
class Discovery:
    start: List[Found] = field(default_factory=list)
    end: List[Found] = field(default_factory=list)
    reads: int = 0                     # reads counted
    windows: int = 0                   # windows counted: one start and one end window per read
    k: int = 12

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


def discover(input_path, k=12, end_size=150, max_reads=None, device=None, aligner=None, adapter_threshold=90.0,
             alignments=False, **assemble_options) -> Discovery:
    """Census, assembly and annotation of one input (file or Albacore directory) -> Discovery.
    max_reads: count only the first so many reads.  aligner: an Aligner of `device` to use (its adapter table is replaced by
    the panel's sequences); default: one of its own.  alignments: every found sequence also gets the alignment against its
    nearest known adapter, drawn (Found.alignment; Aligner.align_pairs_paths).  assemble_options: min_fraction, extend_ratio,
    min_len."""
    import torch
    from . import runner
    from .batch import Aligner, records_to_fields
    from .panel import load_panel
    k, end_size = int(k), int(end_size)
    if not 4 <= k <= 13:
        raise ValueError("Error: k must be between 4 and 13")
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
        every = found[0] + found[1]
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
                _, heads, strings = aligner.align_pairs_paths(list(zip([f.sequence for f in every], bests)))
                for f, best, head, text in zip(every, bests, heads, strings):
                    f.alignment = render_alignment(f.sequence, seqs[best], head, text)
        return Discovery(found[0], found[1], reads=n, windows=2 * n, k=k)
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
    a = p.parse_args(argv)
    try:
        extra = read_adapters(a.extra_adapters) if a.extra_adapters else []
        d = discover(a.input, k=a.k, end_size=a.end_size, max_reads=a.max_reads, adapter_threshold=a.adapter_threshold,
                     min_fraction=a.min_fraction, extend_ratio=a.extend_ratio, min_len=a.min_len, alignments=a.alignments)
    except ValueError as e:
        sys.exit(str(e))
    except RuntimeError as e:
        sys.exit("Error: " + str(e))
    print("\n".join(["side\tsequence\tpeak\tsupport\tshare\tnearest\tidentity\tstatus"] + report_lines(d, a.alignments)))
    new = d.adapter_sets()
    if a.adapters_out:
        write_adapters(a.adapters_out, new)
    if a.output is not None or a.barcode_dir is not None:
        from .panel import load_panel
        run_cli(a, adapter_panel=load_panel() + new + extra)


if __name__ == "__main__":
    main()
