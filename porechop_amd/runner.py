"""End to end: reads in -> adapters found, ends trimmed, barcodes called, chimeras split -> reads out.

This is the batch form of everything porechop/porechop.py:33-79 (main) does around the hot path --
SURVEY.md section 8f rows 2 (per-read orchestration) and 3 (output) -- written against arrays
instead of per-read Python objects:

  loading            porechop.py:216-268   (file, or Albacore directory with per-file check reads
                                            and barcode calls read off the path)  -> io.ReadSet (C++)
  phase A + rules    porechop.py:286-327, 374-390, 330-371, 410-436              -> Pipeline.phase_a, panel.py
  phase B            porechop.py:438-514 + nanopore_read.py:166-208              -> Pipeline.phase_b
  barcode calls      nanopore_read.py:399-473 (determine_barcode)                -> pipeline.call_barcodes     
  phase C            porechop.py:533-595 + nanopore_read.py:210-243              -> Pipeline.phase_c
  pieces to write    nanopore_read.py:56-147 (trim slices, split parts, naming)  -> _plan_pieces (numpy)
  writing            porechop.py:607-734                                         -> ReadSet.write (C++)

The alignments come from the GPU library only (Pipeline's default aligner); output files are
byte-identical to the reference's (tests/test_runner_*.py).  Progress tables and coloured
per-read dumps (verbosity >= 1 in the reference) are not reproduced: run() returns the numbers.
"""
import os
import re
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import panel as panel_rules
from .distributed import gather_in_order, reduce_presence, shard_by_bases
from .io import GzStream, ReadSet, gz_finish
from .pipeline import AdapterSet, DeviceReads, MiddleHits, Pipeline, ScanParams, trimmed_interval


@dataclass
class Options:
    """Defaults of porechop/porechop.py:85-185 (get_arguments)."""
    format: str = "auto"                      # auto | fasta | fastq | fasta.gz | fastq.gz
    barcode_threshold: float = 75.0
    barcode_diff: float = 5.0
    require_two_barcodes: bool = False
    untrimmed: bool = False
    discard_unassigned: bool = False
    adapter_threshold: float = 90.0
    check_reads: int = 10000
    scoring_scheme: Tuple[int, int, int, int] = (3, -6, -5, -2)
    end_size: int = 150
    min_trim_size: int = 4
    extra_end_trim: int = 2
    end_threshold: float = 75.0
    no_split: bool = False
    discard_middle: bool = False
    middle_threshold: float = 90.0
    extra_middle_trim_good_side: int = 10
    extra_middle_trim_bad_side: int = 100
    min_split_read_size: int = 1000


@dataclass
class RunResult:
    n_reads: int = 0
    read_type: str = "FASTQ"
    matching_sets: List[str] = field(default_factory=list)       # after the 1D^2 fix-up and the full barcode sets
    barcode_orientation: Optional[str] = None
    start_trim: Optional[np.ndarray] = None                      # int32 [R]
    end_trim: Optional[np.ndarray] = None
    barcode_calls: Optional[List[str]] = None                    # per read, when binning
    middle_hit_reads: int = 0
    files: Dict[str, Tuple[int, int]] = field(default_factory=dict)   # path -> (records written, bases)
    out_format: str = "fastq"
    seconds: Dict[str, float] = field(default_factory=dict)      # wall-clock per stage
    counts: Dict[str, int] = field(default_factory=dict)         # whole-run tallies where start_trim / end_trim hold one rank's reads
    # a sharded run (run_sharded): start_trim / end_trim / barcode_calls cover THIS rank's reads only -- reads
    # [first_read, first_read + local_reads) of the n_reads of the file; everywhere else first_read = 0, local_reads = n_reads
    first_read: int = 0
    local_reads: Optional[int] = None
    explain: Optional["RunExplain"] = None                       # run(..., report=PATH): why every read was trimmed and called
    # run(..., umi=True): per read (start, end), each None or (set name, first base in the read, length, covered, bases)
    umis: Optional[List[tuple]] = None
    # run(..., umi_groups=PATH): per read None (no key) or (group id from 1, the group's representative key)
    umi_groups: Optional[List[Optional[tuple]]] = None
    # run(..., umi_consensus=PATH): one dict per group, in group order (porechop_amd.consensus.call_groups): group,
    # representative, members, used, rejected, skipped, rounds, length, status, sequence (bytes; None unless status is "called");
    # with umi_consensus_fastq=PATH also quality (bytes of Phred values, one per base of sequence; None without a sequence)
    consensus: Optional[List[dict]] = None


@dataclass
class RunExplain:
    """Host arrays behind the per-read report of run(..., report=PATH), for the reads of the run in input order.  The first
    four are pc_phase_b_explain's outputs (include/porechop_amd.h); the middle hits are those of phase C."""
    summary: np.ndarray                      # int32 [R, 12]
    bscore: np.ndarray                       # float64 [R, 4]
    hit_first: np.ndarray                    # int64 [R + 1]
    hits: np.ndarray                         # int32 [H, 6]: job, read_start, read_end, matches, aligned_len, full_len
    job_side: List[int]                      # job -> 0 (start) / 1 (end)
    job_set: List[str]                       # job -> name of its adapter set
    bin_names: Optional[List[str]]           # None when not demultiplexing
    middle_first: np.ndarray                 # int64 [R + 1]
    middle: np.ndarray                       # int64 [M, 3]: adapter (index into middle_names), read_start, read_end -- trimmed-read
    middle_identity: np.ndarray              # float64 [M]     coordinates, discovery order
    middle_names: List[str]
    albacore: Optional[List[Optional[str]]] = None
    calls: Optional[List[str]] = None        # the final call, after the Albacore rule
    hit_cigars: Optional[List[str]] = None   # run(..., report_paths=True): per row of `hits`, "read_first|adapter_first|CIGAR"
    middle_cigars: Optional[List[str]] = None   # run(..., report_middle_paths=True): per row of `middle`, the same, trimmed-read coordinates

    @staticmethod
    def identity(matches, length):
        """The %f-rounded identity the reference parses from a record with these fields."""
        return float("%f" % ((100.0 * matches) / length)) if length else float("nan")

    def end_alignments(self, r):
        """-> (start list, end list) of (set name, full identity, aligned identity, read_start, read_end): the tuples of the
        reference's start_adapter_alignments / end_adapter_alignments, with the set's name for the set."""
        out = ([], [])
        for j, rs, re, m, al, fl in self.hits[int(self.hit_first[r]):int(self.hit_first[r + 1])].tolist():
            out[self.job_side[j]].append((self.job_set[j], self.identity(m, fl), self.identity(m, al), rs, re))
        return out

    def end_cigars(self, r):
        """-> (start list, end list) of "read_first|adapter_first|CIGAR", entry for entry with end_alignments(r): the path of
        each alignment in the window coordinates its read_start / read_end use."""
        out = ([], [])
        a, b = int(self.hit_first[r]), int(self.hit_first[r + 1])
        for (j, *_), text in zip(self.hits[a:b].tolist(), self.hit_cigars[a:b]):
            out[self.job_side[j]].append(text)
        return out

    def barcodes(self, r):
        """-> ((best start name, identity), (second), (best end), (second)); 'none' / 0.0 as in the reference."""
        return tuple((self.bin_names[k] if k >= 0 else "none", float(v))
                     for k, v in zip(self.summary[r, 6:10].tolist(), self.bscore[r].tolist()))

    def middle_hits(self, r):
        """-> [(adapter name, read_start, read_end, full identity)] in discovery order."""
        a, b = int(self.middle_first[r]), int(self.middle_first[r + 1])
        return [(self.middle_names[ad], s_, e_, float(v)) for (ad, s_, e_), v in zip(self.middle[a:b].tolist(), self.middle_identity[a:b].tolist())]


REPORT_COLUMNS = ["name", "length", "start_trim", "end_trim", "start_alignments", "end_alignments", "middle_hits",
                  "best_start_barcode", "best_start_identity", "second_start_barcode", "second_start_identity",
                  "best_end_barcode", "best_end_identity", "second_end_barcode", "second_end_identity", "albacore_call", "barcode_call"]


REPORT_PATH_COLUMNS = ["start_cigars", "end_cigars"]              # appended by run(..., report_paths=True)
REPORT_MIDDLE_PATH_COLUMNS = ["middle_cigars"]                    # appended (last) by run(..., report_middle_paths=True)


def report_header(paths=False, middle_paths=False):
    return "#" + "\t".join(REPORT_COLUMNS + (REPORT_PATH_COLUMNS if paths else []) + (REPORT_MIDDLE_PATH_COLUMNS if middle_paths else [])) + "\n"


def report_rows(ex: RunExplain, names, lengths):
    """The report's rows for the reads of `ex` (TSV; list columns ';'-joined, '.' when empty or not applicable).  With the
    per-hit paths (ex.hit_cigars) two columns follow: start_cigars / end_cigars, entry for entry with the alignment columns;
    with the middle hits' paths (ex.middle_cigars) one more, middle_cigars, entry for entry with middle_hits."""
    rows = []
    for r in range(ex.summary.shape[0]):
        starts, ends = ex.end_alignments(r)
        fmt_end = lambda xs: ";".join("%s|%.6f|%.6f|%d|%d" % x for x in xs) or "."
        mids = ";".join("%s|%d|%d|%.6f" % x for x in ex.middle_hits(r)) or "."
        cols = [names[r].replace("\t", " "), str(int(lengths[r])), str(int(ex.summary[r, 0])), str(int(ex.summary[r, 1])),
                fmt_end(starts), fmt_end(ends), mids]
        if ex.bin_names is None:
            cols += ["."] * 10
        else:
            for name, v in ex.barcodes(r):
                cols += [name, "%.6f" % v]
            alb = ex.albacore[r] if ex.albacore is not None else None
            cols += [alb if alb is not None else ".", ex.calls[r]]
        if ex.hit_cigars is not None:
            cols += [";".join(xs) or "." for xs in ex.end_cigars(r)]
        if ex.middle_cigars is not None:
            cols.append(";".join(ex.middle_cigars[int(ex.middle_first[r]):int(ex.middle_first[r + 1])]) or ".")
        rows.append("\t".join(cols) + "\n")
    return "".join(rows)


def _chain(firsts, tables):
    """Consecutive blocks of a prefix-indexed table as one: firsts[k] (exclusive prefix sums, n_k + 1 entries) index the rows
    of tables[k] -> (first [sum n_k + 1], rows)."""
    out, base = [np.zeros(1, dtype=np.int64)], 0
    for f in firsts:
        out.append(f[1:] + base)
        base += int(f[-1])
    return np.concatenate(out), np.concatenate(tables)


def _host_explain(parts, R, pl, match_idx, sc, albacore, paths=False):
    """RunExplain of R reads from the EndExplain of every block (in order) and the host results of their scan (sc: _Scan, with
    the middle hits' identities)."""
    hits_h, hits_id = sc.hits, sc.identity
    if parts:
        summary = np.concatenate([e.summary.cpu().numpy() for e in parts])
        bscore = np.concatenate([e.bscore.cpu().numpy() for e in parts])
        hit_first, hits = _chain([e.hit_first.cpu().numpy() for e in parts], [e.hits.cpu().numpy() for e in parts])
        jobs = parts[0].jobs
    else:
        summary = np.zeros((R, 12), dtype=np.int32)
        summary[:, 4:10] = -1
        bscore = np.zeros((R, 4), dtype=np.float64)
        hits, hit_first, jobs = np.zeros((0, 6), dtype=np.int32), np.zeros(R + 1, dtype=np.int64), []
    cigars = None
    if parts and all(e.path_heads is not None for e in parts):
        from .batch import cigar, decode_paths
        cigars = []
        for e in parts:                                               # chained like `hits`
            heads = e.path_heads.cpu().numpy()
            cigars += ["%d|%d|%s" % (int(h[1]), int(h[2]), cigar(t)) for h, t in zip(heads, decode_paths(heads, e.path_ops.cpu().numpy()))]
    elif not parts and paths:
        cigars = []
    order = np.argsort(hits_h[:, 0], kind="stable")                  # per read, in discovery order
    middle_first = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(hits_h[:, 0], minlength=R), out=middle_first[1:])
    return RunExplain(summary, bscore, hit_first, hits, [side for side, _ in jobs], [pl.sets[si].name for _, si in jobs], sc.bin_names,
                      middle_first, hits_h[order][:, 1:4], hits_id[order],
                      [a[0] for a in pl.middle_adapter_list(match_idx)] if match_idx else [], albacore, sc.calls, cigars,
                      None if sc.middle_cigars is None else [sc.middle_cigars[k] for k in order.tolist()])


# (read, adapter) pairs one block of phases B / C may hold at a time: 8 ints each, a few copies -> a few GB of HBM
READ_BLOCK_PAIRS = 64_000_000
MIN_READ_BLOCK = 4096


class UsageError(ValueError):
    """What the reference reports with sys.exit('Error: ...')."""


def _albacore_barcode(path):
    # porechop.py:271-278
    if "/unclassified/" in path:
        return "none"
    m = re.findall(r"/barcode(\d\d)/", path)
    if m:
        return "BC" + m[-1]
    return None


def _load(input_path, check_read_count):
    """-> (ReadSet, check-read indices, per-read Albacore call or None)."""
    if os.path.isfile(input_path):
        rs = ReadSet(input_path)
        return rs, np.arange(min(rs.count, max(0, check_read_count)), dtype=np.int64), None
    if os.path.isdir(input_path):
        fastqs = sorted(os.path.join(d, f) for d, _, fs in os.walk(input_path) for f in fs
                        if f.lower().endswith(".fastq") or f.lower().endswith(".fastq.gz"))
        if not fastqs:
            raise UsageError("Error: could not find fastq files in " + input_path)
        rs = ReadSet(fastqs)
        if not rs.is_fastq:
            raise UsageError("Error: " + fastqs[0] + " is not FASTQ")
        per_file = int(round(check_read_count / len(fastqs)))
        fi = rs.file_index
        first_of_file = np.searchsorted(fi, np.arange(len(fastqs)), side="left")
        rank_in_file = np.arange(rs.count, dtype=np.int64) - first_of_file[fi]
        check = np.nonzero(rank_in_file < per_file)[0].astype(np.int64)
        calls = [_albacore_barcode(p) for p in fastqs]
        return rs, check, [calls[i] for i in fi]
    raise UsageError("Error: could not find " + input_path)


def barcode_bins(pl, bc_sets):
    """-> (bin names, [(start set, end set)] per bin).  The reference's two score dicts are keyed by bin
    name: a later set with the same name overwrites the value but keeps the first insertion's position."""
    names = _bin_names(pl, bc_sets)
    col = {n: k for k, n in enumerate(names)}
    bins = [[None, None] for _ in names]
    for i in bc_sets:
        k = col[panel_rules.barcode_name(pl.sets[i])]
        if pl.sets[i].start is not None:
            bins[k][0] = i
        if pl.sets[i].end is not None:
            bins[k][1] = i
    return names, [tuple(b) for b in bins]


def _bin_names(pl, bc_sets):
    names = []
    for i in bc_sets:
        n = panel_rules.barcode_name(pl.sets[i])
        if n not in names:
            names.append(n)
    return names


def _barcode_bin_names(pl, match_idx, orientation):
    return _bin_names(pl, [i for i in match_idx if panel_rules.is_barcode(pl.sets[i])
                           and panel_rules.barcode_direction(pl.sets[i]) == orientation])


def _split_parts(tlen, intervals, min_size):
    """get_split_read_parts (nanopore_read.py:76-95): positions of the trimmed read not covered by
    any [trim_start, trim_end) -> maximal runs -> those of at least min_size bases."""
    cover = np.zeros(tlen + 1, dtype=np.int32)
    for a, b in intervals:
        a, b = max(a, 0), min(b, tlen)
        if b > a:
            cover[a] += 1
            cover[b] -= 1
    keep = np.cumsum(cover[:tlen]) == 0
    edges = np.diff(np.concatenate([[0], keep.astype(np.int8), [0]]))
    starts, ends = np.nonzero(edges == 1)[0], np.nonzero(edges == -1)[0]
    return [(int(s), int(e - s)) for s, e in zip(starts, ends) if e - s >= min_size]


def _resolve_format(opts: Options, output, barcode_dir, read_type, input_path):
    # porechop.py:627-655
    fmt = opts.format
    if fmt == "auto":
        if output is None:
            fmt = read_type.lower()
            if barcode_dir is not None and input_path.lower().endswith(".gz"):
                fmt += ".gz"
        elif ".fasta.gz" in output.lower():
            fmt = "fasta.gz"
        elif ".fastq.gz" in output.lower():
            fmt = "fastq.gz"
        elif ".fasta" in output.lower():
            fmt = "fasta"
        elif ".fastq" in output.lower():
            fmt = "fastq"
        else:
            fmt = read_type.lower()
    gz = fmt.endswith(".gz") and (barcode_dir is not None or output is not None)
    if gz:
        fmt = fmt[:-3]
    # (to stdout a '.gz' format is left as it is and, not being 'fasta', prints FASTQ -- as there)
    return fmt, gz


def _is_gzip(path):
    # misc.py:60-81 get_compression_type: by magic bytes, not by name
    try:
        with open(path, "rb") as f:
            return f.read(3) == b"\x1f\x8b\x08"
    except OSError:
        return False


def gz_out_hint(opts, output, barcode_dir, input_path):
    """Will this run write gzip?  (_resolve_format before the read type is known: FASTQ assumed.)"""
    try:
        return _resolve_format(opts, output, barcode_dir, "FASTQ", input_path)[1]
    except Exception:
        return False


def _open_pipeline(opts, device, aligner, adapter_panel, wildcards=False, umi=False):
    """-> (adapter panel, Pipeline) for a run's options.  wildcards: IUPAC letters in the panel's adapters stand for their sets of
    bases (ScanParams.wildcards); not an Option -- the options are the reference's.  umi: the run keeps the read bases under the
    adapters' degenerate letters -- a panel none of whose sets has such a letter is a UsageError."""
    panel = list(adapter_panel) if adapter_panel is not None else panel_rules.load_panel()
    params = ScanParams(end_size=opts.end_size, min_trim_size=opts.min_trim_size, extra_end_trim=opts.extra_end_trim,
                        end_threshold=opts.end_threshold, middle_threshold=opts.middle_threshold,
                        adapter_threshold=opts.adapter_threshold, check_reads=opts.check_reads,
                        scores=tuple(int(x) for x in opts.scoring_scheme), wildcards=bool(wildcards))
    pl = Pipeline(panel, params, device=device, aligner=aligner)
    if aligner is None:
        # a one-shot run should not wait for hiprtc: specialised kernels are compiled on a worker
        # thread and picked up by later launches (pc_jit_async, include/porechop_amd.h)
        pl.aligner.lib.pc_jit_async(1)
    if umi and not pl.umi_adapters(range(len(pl.sets))):
        if aligner is None:
            pl.close()
        raise UsageError("Error: --umi needs an adapter with degenerate letters (IUPAC codes such as N, V or R): none of the panel's sets has one")
    return panel, pl


UMI_REPORT_COLUMNS = ["name", "side", "set", "read_first", "length", "covered", "span_length", "umi"]


def umi_report_header():
    return "#" + "\t".join(UMI_REPORT_COLUMNS) + "\n"


def _tag_umis(rs, sc, pl):
    """What run(umi=True) does with the UMIs of a scanned ReadSet before any piece of it is written: the bases are taken from
    the host reads at the coordinates Pipeline.end_umis returned -- the bytes as they stand in the input, in read orientation
    on either side --, every read with one gets UMI_start=<bases> and / or UMI_end=<bases> at the end of its stored header
    (ReadSet.annotate: all pieces of a split read carry them), -> (RunResult.umis for these reads, the rows of the UMI report:
    one per extracted UMI, in read order, start before end).  A side whose span has no read base under it (length 0) has no UMI."""
    R = rs.count
    per_read = [[None, None] for _ in range(R)]
    tagged, texts, rows = [], [], []
    if sc.umis is not None:
        span_len = {(side, si): span[1] - span[0] + 1 for side, si, _ai, span in pl.umi_adapters(range(len(pl.sets)))}
        found = []
        for side, (sets, first, length, covered) in enumerate(sc.umis):
            for r in np.nonzero((sets >= 0) & (length > 0))[0].tolist():
                found.append((r, side, int(sets[r]), int(first[r]), int(length[r]), int(covered[r])))
        found.sort()
        for r, side, si, first, length, covered in found:
            at = int(rs.offsets[r]) + first
            assert 0 <= first and first + length <= int(rs.lengths[r])
            bases = rs.arena[at:at + length].tobytes().decode("latin-1")
            per_read[r][side] = (pl.sets[si].name, first, length, covered, bases)
            tagged.append(r)
            texts.append(("UMI_end=" if side else "UMI_start=") + bases)
            rows.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (rs.name(r).split(" ")[0], "end" if side else "start", pl.sets[si].name, first,
                                                                length, covered, span_len[(side, si)], bases))
        if tagged:
            rs.annotate(tagged, texts)
    return [tuple(x) for x in per_read], "".join(rows)


def _check_umi_group_options(umi, umi_groups, by, max_dist, method):
    """The refusals of run(umi_groups=PATH) that need no panel."""
    from . import umi_groups as ug
    if umi_groups is None:
        return
    if not umi:
        raise UsageError("Error: --umi_groups needs --umi")
    if by is not None and by not in ug.BY:
        raise UsageError("Error: --umi_group_by must be one of start, end, both (got %r)" % (by,))
    if method not in ug.METHODS:
        raise UsageError("Error: --umi_group_method must be one of directional, cluster (got %r)" % (method,))
    if not 0 <= int(max_dist) <= ug.MAX_KEY:
        raise UsageError("Error: --umi_max_dist must lie in 0..%d" % ug.MAX_KEY)


def _check_umi_strand_options(umi, umi_strands, grouping, by):
    """The refusals of run(umi_strands=True) that need no panel."""
    if not umi_strands:
        return
    if not umi:
        raise UsageError("Error: --umi_strands needs --umi")
    if not grouping:
        raise UsageError("Error: --umi_strands needs --umi_groups or --umi_consensus")
    if by is not None and by != "both":
        raise UsageError("Error: --umi_strands needs --umi_group_by both (got %r): the mirror of a one-sided key lies at the read's other "
                         "end, and which end that is belongs to the protocol" % (by,))


def _umi_group_by(pl, by, strands=False):
    """Which UMIs make a read's key: `by` as given when the panel has a span on every side it names (else a UsageError), and for
    None "both" when the panel has spans on both sides, else the side that has one."""
    sides = {side for side, _si, _ai, _span in pl.umi_adapters(range(len(pl.sets)))}
    if strands and sides != {0, 1}:
        raise UsageError("Error: --umi_strands needs degenerate letters in a start and in an end adapter (--umi_group_by both): the panel "
                         "has them on one side only")
    if by is None:
        return "both" if sides == {0, 1} else ("start" if 0 in sides else "end")
    for side, word in ((0, "start"), (1, "end")):
        if by in (word, "both") and side not in sides:
            raise UsageError("Error: --umi_group_by %s needs degenerate letters in a %s adapter: the panel has none there" % (by, word))
    return by


def _group_umis(path, umis, names, pl, by, max_dist, method, max_keys, strands=False):
    """run(umi_groups=PATH) after the last read: the reads' keys, the pairs of distinct keys within max_dist edits -- on the
    GPU when the aligner has umi_neighbours, in numpy otherwise --, the groups (porechop_amd.umi_groups) and the TSV ->
    RunResult.umi_groups.  strands (umi_strands=True): across both strands of a molecule -- the entries gain the read's strand,
    the TSV its eighth column."""
    from . import umi_groups as ug
    strand_kw = dict(strands=True) if strands else {}
    try:
        per_read, rows = ug.assign(umis, names, by, int(max_dist), method, int(max_keys), pl.aligner, pl.device, **strand_kw)
    except OverflowError as e:
        raise UsageError("Error: %s distinct UMI keys are more than --umi_group_max_keys %d allows: the all-against-all pass grows "
                         "with the square of their number; raise --umi_group_max_keys to run it all the same" % (e.args[0], int(max_keys)))
    if path is not None:                                        # run(umi_consensus=PATH) alone makes the groups and writes no TSV
        with open(path, "w") as fh:
            fh.write(ug.groups_header(**strand_kw))
            fh.write(rows)
    return per_read


CONSENSUS_OPTIONS = ("min_reads", "max_reads", "band", "rounds", "max_err_pct", "max_len")


QUALITY_DEFAULTS = dict(vote_err_pct=10, max_qual=60)


def _check_umi_consensus_options(umi, umi_consensus, umi_consensus_report, sharded, values, fastq=None, vote_err_pct=10, max_qual=60):
    """The refusals of run(umi_consensus=PATH) and run(umi_consensus_fastq=PATH) that need no panel; values: the six numeric
    options in CONSENSUS_OPTIONS' order."""
    from . import consensus as cs
    if umi_consensus_report is not None and umi_consensus is None and fastq is None:
        raise UsageError("Error: --umi_consensus_report needs --umi_consensus or --umi_consensus_fastq")
    if fastq is None and (vote_err_pct != QUALITY_DEFAULTS["vote_err_pct"] or max_qual != QUALITY_DEFAULTS["max_qual"]):
        raise UsageError("Error: --umi_consensus_vote_err_pct and --umi_consensus_max_qual need --umi_consensus_fastq")
    if umi_consensus is None and fastq is None:
        return
    if not umi:
        raise UsageError("Error: --umi_consensus%s needs --umi" % ("" if umi_consensus is not None else "_fastq"))
    if fastq is not None:
        for name, v, hi in (("vote_err_pct", vote_err_pct, 50), ("max_qual", max_qual, cs.MAX_QUAL)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
                raise UsageError("Error: --umi_consensus_%s must be a whole number in 1..%d" % (name, hi))
    if sharded:
        raise UsageError("Error: the UMI consensus is not available in a sharded run (one process per GPU): run it in a single process")
    try:
        bad = cs.check_options(*[int(v) for v in values])
    except (TypeError, ValueError):
        bad = ("band", "and the other numeric options must be whole numbers")
    if bad:
        raise UsageError("Error: --umi_consensus_%s %s" % bad)


def _consensus(fasta, report, res, rs, reads, pr, num, pl, values, strands=False, fastq=None, qual_table=None):
    """run(umi_consensus=PATH) after the piece plan: the groups' members (reads written as exactly one piece), the rounds over
    the arena _upload made -- on the library when the aligner has consensus_round, in numpy otherwise -- and the files ->
    RunResult.consensus.  fastq / qual_table (run(umi_consensus_fastq=PATH)): the rounds also leave a quality per base, the
    rows carry `quality`, PATH gets the FASTQ and the report its two quality columns."""
    from . import consensus as cs
    lengths = np.asarray(rs.lengths, dtype=np.int64)
    groups = cs.members(res.umi_groups, lengths, res.start_trim, res.end_trim, pr, num)
    seq_off = np.asarray(rs.offsets, dtype=np.int64) + np.asarray(res.start_trim, dtype=np.int64)
    seq_len = np.maximum(lengths - np.asarray(res.end_trim, dtype=np.int64) - np.asarray(res.start_trim, dtype=np.int64), 0)
    written = []
    strand_kw = dict(read_strand=[0 if e is None else int(e[2]) for e in res.umi_groups]) if strands else {}
    report_kw = dict(minus=True) if strands else {}
    if qual_table is not None:
        strand_kw["qual_table"] = qual_table
        report_kw["quality"] = True
    try:
        out = cs.call_groups(groups, rs.arena, seq_off, seq_len, *[int(v) for v in values], aligner=pl.aligner,
                             dev_arena=reads.arena if reads is not None else None, device=pl.device, **strand_kw)
        for path, text in ((fasta, cs.fasta_text), (fastq, cs.fastq_text), (report, lambda rows: cs.report_text(rows, **report_kw))):
            if path is not None:
                text = text(out)
                written.append(path)
                with open(path, "w") as fh:
                    fh.write(text)
    except Exception:
        for path in written:
            if os.path.isfile(path):
                os.remove(path)
        raise
    return out


def _upload(rs, dev, lo=0, hi=None):
    """Reads [lo, hi) of a ReadSet (default: all of it, None for no ReadSet) on the device -> DeviceReads, None when there are
    none.  A range takes its slice of the arena and 64 bytes past it (>= 16 must be readable past the end: the kernels fetch 16
    columns per load); the whole set takes the whole arena, which ends in that padding."""
    hi = (rs.count if rs is not None else 0) if hi is None else hi
    if hi <= lo:
        return None
    a0 = int(rs.offsets[lo]) if lo else 0
    a1 = rs.arena.size if hi == rs.count else min(int(rs.offsets[hi - 1]) + int(rs.lengths[hi - 1]) + 64, rs.arena.size)
    return DeviceReads(torch.from_numpy(rs.arena[a0:a1]).to(dev), torch.from_numpy(rs.offsets[lo:hi] - a0).to(dev),
                       torch.from_numpy(rs.lengths[lo:hi].copy()).to(dev))


def _piece_files(piece_bins, n_pieces, barcode_dir, single, fmt, gz, known=()):
    """The files of n_pieces pieces -> (bins, file index per piece [int32], paths).  Without bins everything goes to `single`.
    With them (piece_bins: the call of every piece's read) each bin in use is barcode_dir/<bin>.<fmt>[.gz] (porechop.py:657-683):
    the `known` bins first, as they come -- the bins of a streamed run's earlier blocks, the union over the ranks of a sharded
    run -- then the others, sorted."""
    if barcode_dir is None:
        return [], np.zeros(n_pieces, dtype=np.int32), [single]
    bins = list(known)
    bins += sorted(set(piece_bins) - set(bins))
    index = {b: k for k, b in enumerate(bins)}
    pf = np.fromiter((index[b] for b in piece_bins), dtype=np.int32, count=n_pieces)
    return bins, pf, [os.path.join(barcode_dir, b + "." + fmt + (".gz" if gz else "")) for b in bins]


def _tally(pr, pn_, pf, nfiles, read_bases):
    """(reads, bases) per file [int64, nfiles x 2] as the reference reports them: it counts reads, not pieces, and for a bin the
    bases of those reads -- read_bases per read: their end-trimmed, or under --untrimmed whole, lengths (_plan_pieces) -- where
    a single output file (read_bases None) counts the bases of its pieces."""
    out = np.zeros((nfiles, 2), dtype=np.int64)
    for k in range(nfiles):
        sel = pf == k
        rr = np.unique(pr[sel])
        out[k] = rr.size, (pn_[sel] if read_bases is None else read_bases[rr]).sum()
    return out


def _finish_files(paths, gz, file_pos=None):
    """After the last piece: the reference always creates its output file, so one that received nothing (file_pos[k] == 0;
    None: the files exist) is created empty, and a gz file gets its end (io.gz_finish)."""
    for k, path in enumerate(paths):
        if file_pos is not None and file_pos[k] == 0:
            open(path, "wb").close()
        if gz:
            gz_finish(path)


def _emit(rs, pr, ps_, pn_, num, pf, paths, fastq, file_pos, gz, shared=False):
    """Pieces of one read set into their files at file_pos (updated): plain bytes (pc_readset_write_at / _shared), or --
    gz -- formatted and deflated by all cores in memory, then written (pc_readset_compress: what the reference gets from
    `pigz -p <threads>` over a temporary file, porechop.py:640-651,685-729).  A gz file is ended by io.gz_finish."""
    if not gz:
        (rs.write_shared if shared else rs.write_at)(pr, ps_, pn_, num, pf, paths, fastq, file_pos)
        return
    img = rs.compress(pr, ps_, pn_, num, pf, len(paths), fastq)
    try:
        img.write(paths, file_pos, shared=shared)
    finally:
        img.close()


def _find_sets(pl, panel, reads, check_idx, opts, barcode_dir, sharded=False):
    """Phase A over the check reads + the set-level rules (porechop.py:286-436) -> (matching sets incl. the full
    barcode sets, their indices in pl.sets, barcode orientation or None)."""
    dev = pl.device
    if reads is not None and check_idx.size:
        # the pruned search gives the same matching sets and best identities, but the table
        # entries of the side of a set that stays below the threshold are only lower bounds; the
        # barcode-kit choice (porechop.py:343-366) sums BOTH sides of every matching barcode set
        # in its tie-break, so a binning run needs the exact table
        bs, be = pl.phase_a(reads, torch.from_numpy(np.ascontiguousarray(check_idx)).to(dev), prune=barcode_dir is None)
    else:
        bs = torch.zeros(len(panel), dtype=torch.float64, device=dev)
        be = torch.zeros(len(panel), dtype=torch.float64, device=dev)
    if sharded:
        bs, be = reduce_presence(bs, be)                    # nanopore_read.py:159,164 across all ranks' check reads
    bs, be = bs.cpu().numpy(), be.cpu().numpy()
    index_of = {id(s): i for i, s in enumerate(pl.sets)}
    score = lambda s: max(bs[index_of[id(s)]], be[index_of[id(s)]])
    matching = [s for s in panel if "(full sequence)" not in s.name and score(s) >= opts.adapter_threshold]
    matching = panel_rules.fix_up_1d2(matching, score)
    orientation = None
    if barcode_dir is not None:
        try:
            orientation = panel_rules.choose_barcoding_kit(matching, lambda s: bs[index_of[id(s)]],
                                                           lambda s: be[index_of[id(s)]])
        except panel_rules.NoBarcodes as e:
            raise UsageError(str(e))
    with_full = panel_rules.add_full_barcode_sets(panel, matching)
    pl.add_sets(with_full[len(matching):])
    index_of = {id(s): i for i, s in enumerate(pl.sets)}
    matching = with_full
    return matching, [index_of[id(s)] for s in matching], orientation


def _scan_reads(pl, reads, R, match_idx, opts, barcode_dir, orientation, lap=lambda *a, **k: None, explain=None, explain_paths=False,
                middle_paths=None):
    """Phases B (+ barcode calls) and C for R resident reads -> (start_trim, end_trim [device int32], bin index per
    read [numpy int64, -1 = none], MiddleHits or None).
    explain: a list that receives the EndExplain of every block; phase B then runs with every pair traced
    (Pipeline.phase_b_explain) -- the same trims and calls; explain_paths: with the path of every qualifying alignment.
    middle_paths: a list that receives (heads, ops) of Pipeline.middle_hit_paths for every block with middle hits, in the order
    the hits are returned in."""
    dev = pl.device
    start_trim = torch.zeros(R, dtype=torch.int32, device=dev)
    end_trim = torch.zeros(R, dtype=torch.int32, device=dev)
    hits = None
    ci = np.full(R, -1, dtype=np.int64)
    if match_idx and R:
        # ---- phase B (+ barcode calls) ------------------------------------------------
        check_barcodes = barcode_dir is not None
        bc_sets = [i for i in match_idx if check_barcodes and panel_rules.is_barcode(pl.sets[i])
                   and panel_rules.barcode_direction(pl.sets[i]) == orientation]
        # Phases B and C are per read: they run over blocks of reads so that the scratch of a run
        # (8 ints per (read, adapter) pair, all middle adapters at once) is bounded by the block, not by
        # the input -- the reference holds one read's alignments at a time (nanopore_read.py:149-243).
        if check_barcodes:
            bins = barcode_bins(pl, bc_sets)[1]
        n_mid = max(1, len(pl.middle_adapter_list(match_idx)))
        n_end = max(1, 2 * len(match_idx))
        block = max(MIN_READ_BLOCK, int(READ_BLOCK_PAIRS // max(n_mid, n_end)))
        st_parts, et_parts, ci_parts, hit_parts = [], [], [], []
        for b0 in range(0, R, block):
            b1 = min(R, b0 + block)
            sub = reads if (b0 == 0 and b1 == R) else DeviceReads(reads.arena, reads.off[b0:b1], reads.length[b0:b1])
            if explain is not None:
                st_b, et_b, ci_b, ex_b = pl.phase_b_explain(sub, match_idx, bins if check_barcodes else None, opts.barcode_threshold,
                                                            opts.barcode_diff, opts.require_two_barcodes,
                                                            **({"paths": True} if explain_paths else {}))
                explain.append(ex_b)
                if check_barcodes:
                    ci_parts.append(ci_b)
            elif check_barcodes:
                st_b, et_b, ci_b = pl.phase_b_demux(sub, match_idx, bins, opts.barcode_threshold, opts.barcode_diff,
                                                    opts.require_two_barcodes)
                ci_parts.append(ci_b)
            else:
                st_b, et_b = pl.phase_b(sub, match_idx)
            lap("phase_b", sync=True)
            if not opts.no_split:
                # identical hits either way: behind the exact prefilter on the GPU library (most pairs never reach the
                # DP), behind the score bound with an injected test aligner
                fast = getattr(pl.aligner, "fast_prefilter", False)
                hb = pl.phase_c(sub, st_b, et_b, match_idx, prove=not fast, prefilter=fast)
                if hb.read.numel():
                    if middle_paths is not None:                     # (the block's own read numbers: before the shift)
                        middle_paths.append(pl.middle_hit_paths(sub, st_b, et_b, hb)[1:])
                    hb.read = hb.read + b0
                    hit_parts.append(hb)
                lap("phase_c", sync=True)
            st_parts.append(st_b); et_parts.append(et_b)
        start_trim, end_trim = torch.cat(st_parts), torch.cat(et_parts)
        if check_barcodes:
            ci = np.concatenate(ci_parts)
        if not opts.no_split:
            if hit_parts:
                hits = MiddleHits(*(torch.cat([getattr(h_, f) for h_ in hit_parts]) for f in ("read", "adapter", "start", "end", "identity")),
                                  max(h_.rounds for h_ in hit_parts), sum(h_.alignments for h_ in hit_parts))
            else:
                hits = MiddleHits(*(torch.empty(0, dtype=dt, device=dev) for dt in
                                    (torch.int64, torch.int32, torch.int32, torch.int32, torch.float64)))
    return start_trim, end_trim, ci, hits


@dataclass
class _Scan:
    """The per-read results of a scan, on the host."""
    st: np.ndarray                           # int32 [R] start trims
    et: np.ndarray                           # int32 [R] end trims
    hits: np.ndarray                         # int64 [H, 4] middle hits: read, adapter, start, end (trimmed-read coordinates)
    identity: Optional[np.ndarray]           # float64 [H], only for the per-read report
    bin_names: Optional[List[str]]           # None when not demultiplexing
    calls: Optional[List[str]]               # bin name per read, "none" without a call
    middle_cigars: Optional[List[str]] = None   # per row of `hits`, "read_first|adapter_first|CIGAR" (report_middle_paths)
    umis: Optional[list] = None              # run(umi=True): Pipeline.end_umis on the host: per side (set, first, length, covered) [R]


def _scan_to_host(pl, reads, R, match_idx, opts, barcode_dir, orientation, lap=lambda *a, **k: None, explain=None, read_base=0,
                  gather=None, explain_paths=False, middle_paths=False, umi=False):
    """_scan_reads for R resident reads, then everything a run needs of it on the host -> _Scan.  The hits' reads are numbered
    from read_base.  gather: called with the device tensors (start_trim, end_trim, bin index, hits [H, 4]) before they leave the
    device -> the same four for the reads the _Scan is to cover (run() gathers every rank's there).  middle_paths: with the
    path of every middle hit (never together with gather).  umi: with Pipeline.end_umis of the reads, after phase B (never
    together with gather)."""
    dev = pl.device
    mp_parts = [] if middle_paths else None
    start_trim, end_trim, ci, hits = _scan_reads(pl, reads, R, match_idx, opts, barcode_dir, orientation, lap, explain, explain_paths,
                                                 mp_parts)
    umis = None
    if umi and R and match_idx:
        assert gather is None
        umis = pl.end_umis(reads, match_idx)
    if hasattr(pl.aligner, "sync"):
        pl.aligner.sync()
    if umis is not None:
        umis = [tuple(x.cpu().numpy() for x in side) for side in umis]
    if hits is not None and hits.read.numel():
        h = torch.stack([hits.read + read_base, hits.adapter.to(torch.int64), hits.start.to(torch.int64),
                         hits.end.to(torch.int64)], dim=1)
    else:
        h = torch.zeros((0, 4), dtype=torch.int64, device=dev)
    if gather is not None:
        start_trim, end_trim, ci_t, h = gather(start_trim, end_trim, torch.from_numpy(ci).to(dev), h)
        ci = ci_t.cpu().numpy()
    h = h.cpu().numpy()
    identity = None
    if explain is not None:
        identity = hits.identity.cpu().numpy() if h.shape[0] else np.zeros(0, dtype=np.float64)
    names = calls = None
    if barcode_dir is not None:
        names = _barcode_bin_names(pl, match_idx, orientation)            # the same list on every rank
        calls = [names[k] if k >= 0 else "none" for k in ci]
    middle_cigars = None
    if middle_paths:
        from .batch import cigar, decode_paths
        middle_cigars = []
        for heads, ops in mp_parts:                                   # chained like the hits
            heads = heads.cpu().numpy()
            middle_cigars += ["%d|%d|%s" % (int(hd[1]), int(hd[2]), cigar(t)) for hd, t in zip(heads, decode_paths(heads, ops.cpu().numpy()))]
        assert len(middle_cigars) == h.shape[0]
    return _Scan(start_trim.cpu().numpy(), end_trim.cpu().numpy(), h, identity, names, calls, middle_cigars, umis)


def _concat_explain(blocks):
    """One RunExplain for the reads of several consecutive blocks."""
    if len(blocks) == 1:
        return blocks[0]
    cat = lambda name: np.concatenate([getattr(b, name) for b in blocks])
    hit_first, hits = _chain([b.hit_first for b in blocks], [b.hits for b in blocks])
    middle_first, middle = _chain([b.middle_first for b in blocks], [b.middle for b in blocks])
    b0 = next((b for b in blocks if b.job_set), blocks[0])
    return RunExplain(cat("summary"), cat("bscore"), hit_first, hits, b0.job_side, b0.job_set, b0.bin_names,
                      middle_first, middle, cat("middle_identity"), b0.middle_names,
                      None if b0.albacore is None else [a for b in blocks for a in b.albacore],
                      None if b0.calls is None else [c for b in blocks for c in b.calls],
                      None if b0.hit_cigars is None else [c for b in blocks for c in b.hit_cigars],
                      None if b0.middle_cigars is None else [c for b in blocks for c in b.middle_cigars])


def _plan_pieces(opts, barcode_dir, lengths, sc, matching, pl, match_idx):
    """Which pieces of which reads are written (porechop.py:607-734, nanopore_read.py:76-147): lengths per read (numpy), sc =
    their _Scan -> (piece_read, piece_start, piece_len, piece_number, the bases per read that a bin's tally counts (_tally;
    None when not binning), reads with middle hits)."""
    st, et, h, calls = sc.st, sc.et, sc.hits, sc.calls
    discard_middle = opts.discard_middle or barcode_dir is not None          # porechop.py:203-204
    s_pos, e_pos = trimmed_interval(torch.from_numpy(np.ascontiguousarray(lengths).copy()), torch.from_numpy(st), torch.from_numpy(et))
    s_pos, e_pos = s_pos.numpy(), e_pos.numpy()
    tlen = np.maximum(e_pos - s_pos, 0)
    split_of = {}
    if h.shape[0]:
        start_names = {s.start[0] for s in matching if s.start is not None}
        end_names = {s.end[0] for s in matching if s.end is not None}
        good, bad = opts.extra_middle_trim_good_side, opts.extra_middle_trim_bad_side
        ad_names = [a[0] for a in pl.middle_adapter_list(match_idx)]
        lo = np.array([bad if n in start_names else good for n in ad_names], dtype=np.int64)
        hi = np.array([bad if n in end_names else good for n in ad_names], dtype=np.int64)
        for r, a, s, e in h:
            split_of.setdefault(int(r), []).append((int(s - lo[a]), int(e + hi[a])))
    whole = opts.untrimmed
    p_start = np.where(whole, 0, s_pos).astype(np.int64)
    p_len = np.where(whole, lengths, tlen).astype(np.int64)
    emit = p_len > 0                                            # "Don't return empty sequences"
    if split_of:
        emit[np.fromiter(split_of.keys(), dtype=np.int64)] = False
    if barcode_dir is not None and opts.discard_unassigned:
        emit &= np.array([c != "none" for c in calls], dtype=bool)
    # reads with middle hits: dropped when discarding, otherwise split and numbered
    extra = []                                                  # (read, start, len, number)
    if split_of and not discard_middle:
        for r, ivs in split_of.items():
            if barcode_dir is not None and opts.discard_unassigned and calls[r] == "none":
                continue
            for k, (ps, pn) in enumerate(_split_parts(int(tlen[r]), ivs, opts.min_split_read_size)):
                extra.append((r, int(s_pos[r]) + ps, pn, k + 1))
    base_reads = np.nonzero(emit)[0].astype(np.int64)
    if extra:
        ex = np.array(extra, dtype=np.int64)
        pr = np.concatenate([base_reads, ex[:, 0]])
        ps_ = np.concatenate([p_start[base_reads], ex[:, 1]])
        pn_ = np.concatenate([p_len[base_reads], ex[:, 2]])
        num = np.concatenate([np.zeros(base_reads.size, dtype=np.int64), ex[:, 3]])
        order = np.lexsort((num, pr))                           # read order, pieces of a read in order
        pr, ps_, pn_, num = pr[order], ps_[order], pn_[order], num[order]
    else:
        pr, ps_, pn_, num = base_reads, p_start[base_reads], p_len[base_reads], np.zeros(base_reads.size, dtype=np.int64)
    return pr, ps_, pn_, num, p_len if barcode_dir is not None else None, len(split_of)


# A plain FASTQ file larger than this is run as a stream of blocks (run_streamed); PC_STREAM_BLOCK_BYTES overrides
STREAM_BLOCK_BYTES = 1 << 28


def _stream_block_bytes():
    v = os.environ.get("PC_STREAM_BLOCK_BYTES")
    return int(v) if v else STREAM_BLOCK_BYTES


def run_streamed(input_path, output, barcode_dir, opts: Options, device=None, aligner=None,
                 adapter_panel: List[AdapterSet] = None, block_bytes: int = None, report: str = None,
                 report_paths: bool = False, report_middle_paths: bool = False, wildcards: bool = False, umi: bool = False,
                 umi_report: str = None, umi_groups: str = None, umi_group_by: str = None, umi_max_dist: int = 2,
                 umi_group_method: str = "directional", umi_group_max_keys: int = 1 << 20, umi_consensus: str = None,
                 umi_strands: bool = False, umi_consensus_fastq: str = None) -> Optional[RunResult]:
    """run() for a plain FASTQ file as a STREAM of blocks: a loader thread parses block k+1 (pc_readset_load_segment,
    all host cores) while block k is uploaded and scanned on the GPU and a writer thread formats and writes block k-1
    (pc_readset_write_at) -- host memory holds three blocks instead of the input, and ingest, scan and writing overlap.
    Phase A and the set-level rules run once, on the first block, which must hold the check reads.  Everything after
    that is per read in Porechop (phases B and C, barcode calls, splitting, naming), so the output files are the ones
    run() writes.  Plain FASTA files (cut where a line begins with '>') and the gzip forms of both stream the same way.
    report: the per-read report of run(), appended block after block (the same bytes as a whole run's); report_paths and
    report_middle_paths as in run().  umi / umi_report as in run(): every block's reads are tagged before the block goes to
    the writer, the UMI report is appended block after block (the same bytes as a whole run's).  umi_groups and its options
    as in run(): the groups are made after the last block, over the UMIs of all blocks; umi_strands as in run().
    -> None when the input is not streamable (a directory, irregular records, a damaged gzip stream, or a first block
    without the check reads): the caller loads the whole file."""
    import queue
    import threading
    if umi_consensus is not None or umi_consensus_fastq is not None:
        raise UsageError("Error: --umi_consensus%s is not available in a streamed run: the reads must stay resident; use run()" % (
            "" if umi_consensus is not None else "_fastq"))
    _check_umi_group_options(umi, umi_groups, umi_group_by, umi_max_dist, umi_group_method)
    _check_umi_strand_options(umi, umi_strands, umi_groups is not None, umi_group_by)
    block_bytes = block_bytes or _stream_block_bytes()
    size = os.path.getsize(input_path)
    t_start = time.perf_counter()
    # .gz input: a producer thread inflates ahead (sized members on several cores, anything else through zlib) and hands
    # over the same blocks the plain file would be cut into (io.GzStream / pc_gzstream_next)
    gz_in = GzStream(input_path) if _is_gzip(input_path) else None
    # the first block is made large enough to hold the check reads (phase A looks at the first N reads of the file)
    first_bytes = block_bytes
    pos = 0
    if gz_in is not None:
        first = gz_in.next(block_bytes, max(0, opts.check_reads))
        if first is False or first is None:      # neither a regular 4-line FASTQ nor a FASTA stream (damaged, empty): the whole-file loader's case
            gz_in.close()
            return None
    while gz_in is None:
        first, pos = ReadSet.segment(input_path, 0, first_bytes)
        if first is None:
            return None
        if pos >= size or first.count >= max(0, opts.check_reads):
            break
        first.close()
        first_bytes *= 4
    res = RunResult(n_reads=0, read_type="FASTQ" if first.is_fastq else "FASTA")     # (plain FASTA streams too: cut at '>' lines)
    busy = {"load": time.perf_counter() - t_start, "scan": 0.0, "write": 0.0}

    try:
        panel, pl = _open_pipeline(opts, device, aligner, adapter_panel, wildcards, umi)
        try:
            group_by = _umi_group_by(pl, umi_group_by, bool(umi_strands)) if umi_groups is not None else None
        except UsageError:
            if aligner is None:
                pl.close()
            raise
    except UsageError:
        first.close()
        if gz_in is not None:
            gz_in.close()
        raise

    fmt, gz = _resolve_format(opts, output, barcode_dir, res.read_type, input_path)
    res.out_format = fmt
    fastq = fmt != "fasta"
    if barcode_dir is not None:
        os.makedirs(barcode_dir, exist_ok=True)
    # the one file of a run without bins (gz: written compressed as it goes, no temporary file)
    target = None if barcode_dir is not None else output if output is not None else "-"

    # ---- loader: blocks 1.. (block 0 is in hand) ------------------------------------------------------
    loaded = queue.Queue(maxsize=1)
    failure = []
    stop = threading.Event()

    # the loader and the writer work at the same time: each gets about half of the cores this process may use
    from ._lib import load_library
    io_lib = load_library()
    try:
        ncores = len(os.sched_getaffinity(0))
        with open("/sys/fs/cgroup/cpu.max") as f_:
            quota, period = f_.read().split()
        if quota != "max":
            ncores = min(ncores, max(1, int(int(quota) / int(period))))
    except Exception:
        ncores = os.cpu_count() or 2
    share = max(2, min(32, ncores // 2))
    # gz output: deflating is the wall of the run (measured, 16 cores: the writer busy 3.6 s of 3.8 at half the cores, the
    # loader -- even one that inflates -- 1.4 s): three quarters of the cores to the writer
    share_w = max(2, min(48, ncores * 3 // 4)) if gz_out_hint(opts, output, barcode_dir, input_path) else share
    share_l = max(2, ncores - share_w) if share_w != share else share

    def loader():
        p_ = pos
        io_lib.pc_io_set_thread_limit(share_l)
        try:
            while gz_in is not None and not stop.is_set():
                t0 = time.perf_counter()
                rs_ = gz_in.next(block_bytes)
                busy["load"] += time.perf_counter() - t0
                if rs_ is None:
                    break
                if rs_ is False:
                    raise ValueError("Error: " + input_path + " could not be parsed - is it formatted correctly?")
                loaded.put(rs_)
            while gz_in is None and p_ < size and not stop.is_set():
                t0 = time.perf_counter()
                rs_, nxt = ReadSet.segment(input_path, p_, block_bytes)
                busy["load"] += time.perf_counter() - t0
                if rs_ is None or nxt <= p_:
                    raise ValueError("Error: " + input_path + " could not be parsed - is it formatted correctly?")
                p_ = nxt
                loaded.put(rs_)
        except BaseException as e:           # noqa: handed to the main thread
            failure.append(e)
        loaded.put(None)

    # ---- writer ---------------------------------------------------------------------------------------
    to_write = queue.Queue(maxsize=1)
    bins, paths, file_pos, tally = [], [], np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.int64)

    def writer():
        nonlocal bins, paths, file_pos, tally
        io_lib.pc_io_set_thread_limit(share_w)
        try:
            while True:
                item = to_write.get()
                if item is None:
                    return
                rs_, pr, ps_, pn_, num, piece_bins, read_bases = item
                t0 = time.perf_counter()
                # the files so far keep their places: a bin first seen in this block follows them
                bins, pf, paths = _piece_files(piece_bins, pr.size, barcode_dir, target, fmt, gz, known=bins)
                new = len(paths) - file_pos.size
                file_pos = np.concatenate([file_pos, np.zeros(new, dtype=np.int64)])
                tally = np.concatenate([tally, np.zeros((new, 2), dtype=np.int64)])
                if pr.size:
                    t1 = time.perf_counter()
                    _emit(rs_, pr, ps_, pn_, num, pf, paths, fastq, file_pos, gz)
                    busy["write_call"] = busy.get("write_call", 0.0) + time.perf_counter() - t1
                tally += _tally(pr, pn_, pf, len(paths), read_bases)
                t1 = time.perf_counter()
                rs_.close()
                busy["free"] = busy.get("free", 0.0) + time.perf_counter() - t1
                busy["write"] += time.perf_counter() - t0
        except BaseException as e:           # noqa
            failure.append(e)
            while to_write.get() is not None:
                pass

    lt = threading.Thread(target=loader, daemon=True)
    wt = threading.Thread(target=writer, daemon=True)
    lt.start(); wt.start()
    st_all, et_all, calls_all = [], [], []
    matching = match_idx = orientation = None
    report_fh, ex_blocks = None, []
    umi_fh, umis_all = None, []
    names_all, groups_all = [], None
    try:
        if report is not None:
            report_fh = open(report, "w")
            report_fh.write(report_header(report_paths, report_middle_paths))
        if umi_report is not None:
            umi_fh = open(umi_report, "w")
            umi_fh.write(umi_report_header())
        rs = first
        while rs is not None:
            if failure:
                break
            t0 = time.perf_counter()
            R = rs.count
            reads = _upload(rs, pl.device)
            if matching is None:
                check_idx = np.arange(min(R, max(0, opts.check_reads)), dtype=np.int64)
                matching, match_idx, orientation = _find_sets(pl, panel, reads, check_idx, opts, barcode_dir)
                res.matching_sets = [s.name for s in matching]
                res.barcode_orientation = orientation
            ex_parts = [] if report is not None else None
            sc = _scan_to_host(pl, reads, R, match_idx, opts, barcode_dir, orientation, explain=ex_parts, explain_paths=report_paths,
                               middle_paths=report_middle_paths, umi=umi)
            if barcode_dir is not None:
                calls_all.extend(sc.calls)
            if report is not None:
                ex = _host_explain(ex_parts, R, pl, match_idx, sc, None, report_paths)
                report_fh.write(report_rows(ex, [rs.name(i) for i in range(R)], rs.lengths))
                ex_blocks.append(ex)
            if umi_groups is not None:
                names_all.extend(rs.name(i).split(" ")[0] for i in range(R))
            if umi:
                block_umis, umi_rows = _tag_umis(rs, sc, pl)
                umis_all.extend(block_umis)
                if umi_fh is not None:
                    umi_fh.write(umi_rows)
            pr, ps_, pn_, num, read_bases, n_split = _plan_pieces(opts, barcode_dir, rs.lengths, sc, matching, pl, match_idx)
            res.middle_hit_reads += n_split
            res.n_reads += R
            st_all.append(sc.st); et_all.append(sc.et)
            piece_bins = [sc.calls[r] for r in pr] if barcode_dir is not None else None
            del reads
            busy["scan"] += time.perf_counter() - t0
            to_write.put((rs, pr, ps_, pn_, num, piece_bins, read_bases))
            rs = loaded.get()
        if umi_groups is not None and not failure:
            try:
                groups_all = _group_umis(umi_groups, umis_all, names_all, pl, group_by, umi_max_dist, umi_group_method, umi_group_max_keys,
                                         bool(umi_strands))
            except UsageError as e:                      # too many keys: like any failure part-way, nothing is left behind
                failure.append(e)
    finally:
        stop.set()
        to_write.put(None)
        wt.join()
        while lt.is_alive() or not loaded.empty():   # blocks the loader had in flight when we stopped early
            try:
                x = loaded.get(timeout=0.05)
                if x is not None:
                    x.close()
            except queue.Empty:
                pass
        if aligner is None:
            pl.close()
        if gz_in is not None:
            gz_in.close()
        if report_fh is not None:
            report_fh.close()
        if umi_fh is not None:
            umi_fh.close()
    if report is not None and ex_blocks:
        res.explain = _concat_explain(ex_blocks)
    if umi:
        res.umis = umis_all
    if umi_groups is not None:
        res.umi_groups = groups_all
    if failure:
        # a streamed run that fails part-way (a later block that cannot be parsed, a full disk) has already written the
        # earlier blocks: a whole-file run would have written nothing, so nothing is left behind here either
        for path in list(paths) + ([report] if report is not None else []) + ([umi_report] if umi_report is not None else []) + (
                [umi_groups] if umi_groups is not None else []):
            try:
                if path and path != "-" and os.path.isfile(path):
                    os.remove(path)
            except OSError:
                pass
        raise failure[0]
    res.start_trim = np.concatenate(st_all) if st_all else np.zeros(0, dtype=np.int32)
    res.end_trim = np.concatenate(et_all) if et_all else np.zeros(0, dtype=np.int32)
    res.barcode_calls = calls_all if barcode_dir is not None else None
    # ---- what a whole-file run does after writing -------------------------------------------------------
    if target != "-":
        _finish_files(paths, gz, file_pos)
        res.files.update(zip(paths, map(tuple, tally.tolist())))
    res.seconds = {"wall": time.perf_counter() - t_start, "load_busy": busy["load"], "scan_busy": busy["scan"], "write_busy": busy["write"],
                   "write_call_busy": busy.get("write_call", 0.0), "free_busy": busy.get("free", 0.0)}
    return res


def run_sharded(input_path, output, barcode_dir, opts: Options, device=None, aligner=None,
                adapter_panel: List[AdapterSet] = None, wildcards: bool = False) -> Optional[RunResult]:
    """One plain FASTQ file -- or one gzip file of sized members, addressed by its inflated bytes -- over the ranks of a
    torch.distributed job WITHOUT any rank touching the whole file: rank r
    parses the records that start in its W-th of the file's bytes (pc_fastq_find_record / pc_readset_load_segment),
    scans them on its GPU and writes its own span of the shared output files (pc_readset_write_sizes, exchanged, give
    every rank its positions; pc_readset_write_shared).  The collectives: phase A's presence table (MAX), read counts,
    output sizes, the names of the bins in use.  The files are the single-process ones byte for byte -- Porechop's
    decisions are per read once the presence table is known (porechop.py:224-273,607-734).
    -> None when this route does not apply on EVERY rank (input not a streamable plain FASTQ file; output to stdout; the
    ranks were given different paths): run() then falls back to every rank loading the input and rank 0 writing."""
    import torch.distributed as dist
    from .distributed import all_agree, all_gather_ints, all_gather_objects
    from .io import fastq_record_start
    rank, world = dist.get_rank(), dist.get_world_size()
    t_start = time.perf_counter()
    target_dir_or_file = os.path.abspath(barcode_dir if barcode_dir is not None else output) if (barcode_dir or output) else None
    ok = os.path.isfile(input_path) and target_dir_or_file is not None
    # the same files on every rank?  (tests run the ranks on private copies: those runs gather to rank 0 as before)
    seen = all_gather_objects((os.path.abspath(input_path), target_dir_or_file, os.path.getsize(input_path) if ok else -1))
    ok = ok and all(x == seen[0] for x in seen)
    rs, b0, b1 = None, 0, 0
    if ok and _is_gzip(input_path):
        # a gzip file of SIZED members (this package's own output; bgzip): positions are those of the inflated bytes, a rank
        # inflates only the members that hold its records (pc_gz_sized_find_record / pc_readset_load_gz_range); any other
        # gzip file cannot be cut without inflating all of it: not this route
        from .io import gz_member_start, gz_sized_record_start, gz_sized_size
        size = gz_sized_size(input_path)
        if not size:
            # an ordinary multi-member gzip file (`cat *.fastq.gz`): cut at MEMBER starts of the compressed bytes -- rank r takes
            # the members that start in its W-th (pc_gz_member_start validates a start by inflating the member behind it) and
            # inflates them with its own cores (GzStream over that byte range); the members must hold whole records (they do when
            # they were files).  ONE member: rank 0 gets all of it, the route still applies (the other ranks write nothing).
            csize = os.path.getsize(input_path)
            b0 = 0 if rank == 0 else gz_member_start(input_path, csize * rank // world)
            b1 = csize if rank == world - 1 else gz_member_start(input_path, csize * (rank + 1) // world)
            if b0 is None or b1 is None:
                ok = False
            elif b1 > b0:
                try:
                    gzs = GzStream(input_path, b0, b1)
                    got = gzs.next(1 << 62, 0)
                    gzs.close()
                except ValueError:
                    got = False
                if got is False:
                    ok = False
                else:
                    rs = got                      # (None: members without a record)
        else:
            b0 = 0 if rank == 0 else gz_sized_record_start(input_path, size * rank // world)
            b1 = size if rank == world - 1 else gz_sized_record_start(input_path, size * (rank + 1) // world)
            if b0 is None or b1 is None:
                ok = False
            elif b1 > b0:
                rs = ReadSet.gz_range(input_path, b0, b1)
                if rs is None:
                    ok = False
    elif ok:
        size = os.path.getsize(input_path)
        b0 = 0 if rank == 0 else fastq_record_start(input_path, size * rank // world)
        b1 = size if rank == world - 1 else fastq_record_start(input_path, size * (rank + 1) // world)
        if b0 is None or b1 is None:
            ok = False
        elif b1 > b0:
            rs, nxt = ReadSet.segment(input_path, b0, b1 - b0)
            if rs is None or nxt != b1:
                ok = False
    if not all_agree(ok, device if aligner is None else None):
        if rs is not None:
            rs.close()
        return None
    R = rs.count if rs is not None else 0
    counts = all_gather_ints([R], device if aligner is None else None)[:, 0].numpy()
    first_read, total = int(counts[:rank].sum()), int(counts.sum())
    # (the type of the file is the type of its first record: rank 0's share always holds it)
    kinds = all_gather_objects(None if rs is None else bool(rs.is_fastq))
    is_fastq = next((k for k in kinds if k is not None), True)
    res = RunResult(n_reads=total, read_type="FASTQ" if is_fastq else "FASTA")
    res.seconds["load"] = time.perf_counter() - t_start
    check_idx = np.arange(max(0, min(R, max(0, opts.check_reads) - first_read)), dtype=np.int64)

    panel, pl = _open_pipeline(opts, device, aligner, adapter_panel, wildcards)
    coll_dev = pl.device if aligner is None else None
    try:
        t0 = time.perf_counter()
        reads = _upload(rs, pl.device)
        matching, match_idx, orientation = _find_sets(pl, panel, reads, check_idx, opts, barcode_dir, sharded=True)
        res.matching_sets = [s.name for s in matching]
        res.barcode_orientation = orientation
        sc = _scan_to_host(pl, reads, R, match_idx, opts, barcode_dir, orientation)
        res.start_trim, res.end_trim, res.barcode_calls = sc.st, sc.et, sc.calls          # this rank's reads
        res.first_read, res.local_reads = first_read, R
        res.seconds["scan"] = time.perf_counter() - t0

        # ---- this rank's pieces, the files they go to, and where ------------------------------------------
        t0 = time.perf_counter()
        fmt, gz = _resolve_format(opts, output, barcode_dir, res.read_type, input_path)
        res.out_format = fmt
        fastq = fmt != "fasta"
        lengths = rs.lengths if R else np.zeros(0, dtype=np.int32)
        pr, ps_, pn_, num, read_bases, n_split = _plan_pieces(opts, barcode_dir, lengths, sc, matching, pl, match_idx)
        tallies = all_gather_ints([n_split, int((sc.st > 0).sum()), int((sc.et > 0).sum())], coll_dev).sum(dim=0)
        res.middle_hit_reads = int(tallies[0])
        res.counts = {"start_trimmed": int(tallies[1]), "end_trimmed": int(tallies[2])}
        piece_bins = everyones = None
        if barcode_dir is not None:
            piece_bins = [sc.calls[r] for r in pr.tolist()]
            everyones = sorted(set().union(*all_gather_objects(sorted(set(piece_bins)))))     # the same files, in the same order, on every rank
        _, pf, paths = _piece_files(piece_bins, pr.size, barcode_dir, output, fmt, gz, known=everyones)
        nf = len(paths)
        # gz: every rank deflates its own pieces in memory first (independent members: any concatenation of them is a valid
        # file), the COMPRESSED sizes are what the ranks exchange, and each writes its image at its position
        img = None
        failed = None
        try:
            if gz and R and nf:
                img = rs.compress(pr, ps_, pn_, num, pf, nf, fastq)
                sizes = img.sizes()[0]
            else:
                sizes = rs.write_sizes(pr, ps_, pn_, num, pf, nf, fastq) if (R and nf) else np.zeros(nf, dtype=np.int64)
        except OSError as e:
            failed, sizes = e, np.zeros(nf, dtype=np.int64)
        # per file: bytes, reads and bases of every rank
        per_file = np.concatenate([np.asarray(sizes, dtype=np.int64).reshape(nf, 1), _tally(pr, pn_, pf, nf, read_bases)], axis=1)
        everyone = all_gather_ints(per_file.reshape(-1), coll_dev).numpy().reshape(world, nf, 3) if nf else np.zeros((world, 0, 3), dtype=np.int64)
        pos = everyone[:rank, :, 0].sum(axis=0).astype(np.int64)
        if rank == 0:
            if barcode_dir is not None:
                os.makedirs(barcode_dir, exist_ok=True)
            for path in paths:
                open(path, "wb").close()                 # created / truncated ONCE, before any rank writes its span
        dist.barrier()
        # a rank that fails here alone (a full disk, a vanished directory) must not leave the others waiting in the
        # next collective: the outcome is exchanged, every rank raises, rank 0 removes the partial files
        try:
            if failed is None and R and pr.size:
                if img is not None:
                    img.write(paths, np.ascontiguousarray(pos), shared=True)
                else:
                    rs.write_shared(pr, ps_, pn_, num, pf, paths, fastq, np.ascontiguousarray(pos))
        except OSError as e:
            failed = e
        finally:
            if img is not None:
                img.close()
        totals = everyone.sum(axis=0)
        if not all_agree(failed is None, coll_dev):
            if rank == 0:
                for path in paths:
                    try:
                        os.remove(path)
                    except OSError:
                        pass
            raise failed if failed is not None else OSError("Error: could not write the output reads (another rank failed)")
        if rank == 0:
            _finish_files(paths, gz)
        res.files.update(zip(paths, map(tuple, totals[:, 1:3].tolist())))
        dist.barrier()
        res.seconds["write"] = time.perf_counter() - t0
        res.seconds["wall"] = time.perf_counter() - t_start
        return res
    finally:
        if aligner is None:
            pl.close()
        if rs is not None:
            rs.close()


def run(input_path, output=None, barcode_dir=None, options: Options = None, device=None, aligner=None,
        adapter_panel: List[AdapterSet] = None, report: str = None, report_paths: bool = False,
        report_middle_paths: bool = False, wildcards: bool = False, umi: bool = False, umi_report: str = None,
        umi_groups: str = None, umi_group_by: str = None, umi_max_dist: int = 2, umi_group_method: str = "directional",
        umi_group_max_keys: int = 1 << 20, umi_consensus: str = None, umi_consensus_report: str = None,
        umi_consensus_min_reads: int = 3, umi_consensus_max_reads: int = 256, umi_consensus_band: int = 64, umi_consensus_rounds: int = 2,
        umi_consensus_max_err_pct: int = 30, umi_consensus_max_len: int = 65535, umi_strands: bool = False,
        umi_consensus_fastq: str = None, umi_consensus_vote_err_pct: int = 10, umi_consensus_max_qual: int = 60) -> RunResult:
    """Porechop's main() on arrays.  output=None and barcode_dir=None writes to stdout.
    `aligner` is for tests only (see Pipeline).

    wildcards=True reads the IUPAC letters of the panel's adapters as their sets of bases (Aligner.set_wildcards; DESIGN.md
    section 15): for custom panels (adapter_panel, python -m porechop_amd.custom).  Off, every byte written is what it is
    without the keyword.

    report=PATH writes the per-read explain report (REPORT_COLUMNS: the qualifying end alignments, the barcode scores and
    the middle hits behind every trim and call, one TSV row per read in input order) and fills RunResult.explain.  Phase B
    then runs with every pair traced (Pipeline.phase_b_explain); trims, calls and output files are the same bytes as
    without it.  Not available in a sharded run.
    report_paths=True appends two columns, start_cigars and end_cigars: per entry of start_alignments / end_alignments its
    path as read_first|adapter_first|CIGAR (= X I D run lengths; the adapter plays SAM's reference), in the window
    coordinates of the entry's read_start / read_end (Pipeline.phase_b_explain(paths=True), Aligner.align_paths).  Without
    it the report is byte for byte the one above.
    report_middle_paths=True appends ONE column, middle_cigars (after start_cigars / end_cigars when both are asked for): per
    entry of middle_hits its path as read_first|adapter_first|CIGAR in trimmed-read coordinates, against the read masked as
    its round of mask-and-realign saw it (Pipeline.middle_hit_paths, Aligner.middle_paths).  Without
    it every report is byte for byte what it is without this option.

    umi=True (with wildcards=True) keeps the UMIs the trim would throw away: the read bases under the degenerate letters of
    the matching sets' start and end adapters (Pipeline.end_umis), taken from the input as they stand
    -- the end side is NOT reverse-complemented.  A read with one gets UMI_start=<bases> and / or UMI_end=<bases> at the end of
    its header, on every piece written of it; RunResult.umis holds, per read, (start, end), each None or (set name, first
    base in the read, length, covered span rows, bases).  umi_report=PATH writes one TSV row per extracted UMI
    (UMI_REPORT_COLUMNS, a '#' header line), in input order, start before end.  Trims, calls and sequences are what they are
    without the option; off, so is every byte.  Not available in a sharded run.

    umi_groups=PATH (with umi=True) says which reads come from one molecule (porechop_amd.umi_groups).  A
    read's key is its UMI of the side umi_group_by names ("start", "end", or "both": START+END, for reads that have both;
    None: "both" when the panel has degenerate letters on both sides, else the side that has them), upper-cased with U -> T.
    The distinct keys are the nodes; two are a pair when their edit distance is <= umi_max_dist (Aligner.umi_neighbours: all
    against all on the GPU); a key that is empty, above 64 bases or holds a letter outside A C G T has no pairs.
    umi_group_method "directional": by count descending, then key, a node not yet grouped founds a group and takes what it
    reaches over pairs with count(a) >= 2 count(b) - 1; "cluster": connected components.  PATH gets a '#' header line and one
    row per read with a key, in input order (umi_groups.GROUP_COLUMNS); RunResult.umi_groups holds, per read, None or
    (group, representative).  More linkable distinct keys than umi_group_max_keys are a UsageError, and then nothing is
    written.  Headers are not tagged with the group: a streamed run has written its blocks before the last UMI is known.

    umi_consensus=PATH (with umi=True) writes ONE CONSENSUS SEQUENCE PER GROUP of reads (porechop_amd.consensus; DESIGN.md section
    18).  The groups are made with the grouping options above whether or not umi_groups=PATH is given (the groups TSV is written
    only when it is).  A group's members are its reads that are written as exactly one piece with at least one base left, as
    their trimmed sequences; a group of at least umi_consensus_min_reads members is called from its first umi_consensus_max_reads
    members: the lower-median member is the template, every other member is aligned to it inside umi_consensus_band (a member
    more than umi_consensus_max_err_pct percent away sits the round out), the alignments vote per column and insertion slot,
    and the call is the template of the next of umi_consensus_rounds rounds.  PATH gets a FASTA record per called group
    (">umi_group_<id> key=<representative> reads=<members> used=<accepted in the last round> rounds=<r> length=<L>"),
    umi_consensus_report=PATH a TSV with one row per group (consensus.REPORT_COLUMNS, a '#' header line) that says why a group
    has no sequence; RunResult.consensus holds both.  The rounds run over the arena already on the device (Aligner.
    consensus_round), so with umi_consensus given run() takes this plain driver whatever the input's size: the reads must be
    resident.  Not available in run_streamed or in a sharded run.  Off, every byte and every launch is what it was.

    umi_consensus_fastq=PATH (with umi=True; alone or beside umi_consensus, either one makes the consensus run) writes the same
    records as FASTQ, with ONE QUALITY VALUE PER BASE: the Phred value that consensus.quality_table(umi_consensus_vote_err_pct,
    umi_consensus_max_qual) gives the base's vote margin -- its votes less those of the strongest alternative (DESIGN.md section
    18; Aligner.consensus_round(qual_table=...)).  RunResult.consensus rows then carry `quality` (bytes of Phred values) and
    the report two more columns, expected_errors and low_qual.  umi_consensus_vote_err_pct (1..50, default 10) and
    umi_consensus_max_qual (1..93, default 60) are choices, not measurements; a value other than the default without
    umi_consensus_fastq is a UsageError.
    umi_strands=True (with umi=True, umi_groups or umi_consensus, and START+END keys: umi_group_by "both" or None on a panel with
    degenerate letters on both sides) groups and calls ACROSS BOTH STRANDS of a molecule (DESIGN.md sections 17 and 18).  A read of
    the minus strand shows the key START+END as rc(END)+rc(START), its mirror; the panel must list the UMI adapter in both
    orientations, as two sets, for such reads to have UMIs at all.  The nodes are the distinct canonical keys (the smaller of a
    key and its mirror, counts summed over both), two keys are a pair when they are within umi_max_dist as they stand or with
    one of them mirrored (Aligner.umi_neighbours(strands=True)), and every read gets a strand: + is the orientation of its
    group's founding canonical key, - the other.  The groups TSV keeps its seven columns with the key as read and gains an
    eighth, strand; RunResult.umi_groups entries become (group, representative, strand 0 / 1).  The consensus piles the - reads
    up as their reverse complements (Aligner.consensus_round(member_strand=...)), every sequence written is in the group's +
    orientation, the FASTA header gains minus=<members read as reverse complement> after reads=, the report TSV a minus
    column, RunResult.consensus dicts `minus`.  Headers of written reads are not changed and reads are not re-oriented.  Off,
    every byte and every launch is what it was.

    Under torch.distributed (one process per GPU) the reads are sharded over the ranks and the adapter-set presence
    table of phase A is MAX-all-reduced (the only cross-read quantity in Porechop).  A plain FASTQ or FASTA file, a gzip
    file of sized members and a `cat` of gzip members take run_sharded: every rank parses, scans and WRITES only its own
    byte range of the input / span of the shared output files, and its RunResult holds its own reads' trims (first_read,
    local_reads say which).  Anything else (one big gzip member, a directory, stdout) falls back to every rank loading the input, contiguous blocks of about equal bases per
    rank, the per-read results gathered in rank order and rank 0 alone planning and writing.  Either way the files
    are the single-process ones."""
    opts = options or Options()
    if len(tuple(opts.scoring_scheme)) != 4:
        raise UsageError("Error: incorrectly formatted scoring scheme")
    if barcode_dir is not None and output is not None:
        raise UsageError("Error: only one of the following options may be used: --output, --barcode_dir")
    if opts.untrimmed and barcode_dir is None:
        raise UsageError("Error: --untrimmed can only be used with --barcode_dir")
    input_path = str(input_path)

    import torch.distributed as dist
    sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1     # one process per GPU
    if report_paths and report is None:
        raise UsageError("Error: --report_paths needs --report")
    if report_middle_paths and report is None:
        raise UsageError("Error: --report_middle_paths needs --report")
    if report is not None and sharded:
        raise UsageError("Error: the per-read report is not available in a sharded run (one process per GPU): run it in a single process")
    if umi and not wildcards:
        raise UsageError("Error: --umi needs --wildcards")
    if umi_report is not None and not umi:
        raise UsageError("Error: --umi_report needs --umi")
    if umi and sharded:
        raise UsageError("Error: UMI extraction is not available in a sharded run (one process per GPU): run it in a single process")
    _check_umi_group_options(umi, umi_groups, umi_group_by, umi_max_dist, umi_group_method)
    consensus_values = (umi_consensus_min_reads, umi_consensus_max_reads, umi_consensus_band, umi_consensus_rounds, umi_consensus_max_err_pct,
                        umi_consensus_max_len)
    _check_umi_consensus_options(umi, umi_consensus, umi_consensus_report, sharded, consensus_values, umi_consensus_fastq,
                                 umi_consensus_vote_err_pct, umi_consensus_max_qual)
    consensing = umi_consensus is not None or umi_consensus_fastq is not None
    if consensing and umi_groups is None:         # the groups are made all the same; only the TSV is not written
        _check_umi_group_options(umi, "", umi_group_by, umi_max_dist, umi_group_method)
    grouping = umi_groups is not None or consensing
    _check_umi_strand_options(umi, umi_strands, grouping, umi_group_by)
    group_kw = {} if umi_groups is None else dict(umi_groups=umi_groups, umi_group_by=umi_group_by, umi_max_dist=umi_max_dist,
                                                  umi_group_method=umi_group_method, umi_group_max_keys=umi_group_max_keys)
    if umi_strands:
        group_kw["umi_strands"] = True
    # (a .gz file holds about three times its size in FASTQ)
    if (os.path.isfile(input_path) and os.path.getsize(input_path) * (3 if _is_gzip(input_path) else 1) > 2 * _stream_block_bytes()
            and not sharded and not consensing):
        streamed = run_streamed(input_path, output, barcode_dir, opts, device=device, aligner=aligner, adapter_panel=adapter_panel,
                                report=report, report_paths=report_paths, report_middle_paths=report_middle_paths, wildcards=wildcards,
                                umi=umi, umi_report=umi_report, **group_kw)
        if streamed is not None:
            return streamed

    if sharded:
        shared = run_sharded(input_path, output, barcode_dir, opts, device=device, aligner=aligner, adapter_panel=adapter_panel,
                             wildcards=wildcards)
        if shared is not None:
            return shared

    t_last = [time.perf_counter()]

    def lap(stage, sync=False):
        if sync and aligner is None and torch.cuda.is_available():
            torch.cuda.synchronize()
        now = time.perf_counter()
        res.seconds[stage] = res.seconds.get(stage, 0.0) + now - t_last[0]
        t_last[0] = now

    rs, check_idx, albacore = _load(input_path, opts.check_reads)
    res = RunResult(n_reads=rs.count, read_type="FASTQ" if rs.is_fastq else "FASTA")
    R_all = rs.count
    rank, world = (dist.get_rank(), dist.get_world_size()) if sharded else (0, 1)
    lo_r, hi_r = shard_by_bases(rs.lengths, world, rank)
    R = hi_r - lo_r                                             # reads this rank scans
    check_idx = check_idx[(check_idx >= lo_r) & (check_idx < hi_r)] - lo_r
    lap("load")

    try:
        panel, pl = _open_pipeline(opts, device, aligner, adapter_panel, wildcards, umi)
        try:
            group_by = _umi_group_by(pl, umi_group_by, bool(umi_strands)) if grouping else None
        except UsageError:
            if aligner is None:
                pl.close()
            raise
    except UsageError:
        rs.close()
        raise
    try:
        reads = _upload(rs, pl.device, lo_r, hi_r)
        lap("upload", sync=True)

        # ---- phase A and the set-level rules ---------------------------------------------
        matching, match_idx, orientation = _find_sets(pl, panel, reads, check_idx if R else np.zeros(0, dtype=np.int64), opts,
                                                      barcode_dir, sharded)
        res.matching_sets = [s.name for s in matching]
        res.barcode_orientation = orientation
        lap("phase_a", sync=True)

        # ---- phases B and C; the per-read results of all ranks, in read order ---------------
        def gather(*tensors):
            tensors = tuple(gather_in_order(x) for x in tensors)
            lap("gather", sync=True)
            return tensors

        ex_parts = [] if report is not None else None
        sc = _scan_to_host(pl, reads, R, match_idx, opts, barcode_dir, orientation, lap, ex_parts, read_base=lo_r,
                           gather=gather if sharded else None, explain_paths=report_paths, middle_paths=report_middle_paths, umi=umi)
        if rank != 0:
            res.start_trim, res.end_trim = sc.st, sc.et
            return res                                           # rank 0 writes
        R = R_all
        if albacore is not None and sc.calls is not None:          # nanopore_read.py:468-473
            sc.calls = [c if (a is None or a == c) else "none" for c, a in zip(sc.calls, albacore)]
        res.start_trim, res.end_trim, res.barcode_calls = sc.st, sc.et, sc.calls
        if report is not None:
            res.explain = _host_explain(ex_parts, R, pl, match_idx, sc, albacore, report_paths)
            with open(report, "w") as fh:
                fh.write(report_header(report_paths, report_middle_paths))
                fh.write(report_rows(res.explain, [rs.name(i) for i in range(R)], rs.lengths))
            lap("report")
        if umi:
            res.umis, umi_rows = _tag_umis(rs, sc, pl)
            if umi_report is not None:
                with open(umi_report, "w") as fh:
                    fh.write(umi_report_header())
                    fh.write(umi_rows)
            lap("umi")
        if grouping:
            res.umi_groups = _group_umis(umi_groups, res.umis, [rs.name(i).split(" ")[0] for i in range(R)], pl, group_by, umi_max_dist,
                                         umi_group_method, umi_group_max_keys, bool(umi_strands))
            lap("umi_groups")

        # ---- which pieces of which reads -------------------------------------------------
        fmt, gz = _resolve_format(opts, output, barcode_dir, res.read_type, input_path)
        res.out_format = fmt
        pr, ps_, pn_, num, read_bases, n_split = _plan_pieces(opts, barcode_dir, rs.lengths, sc, matching, pl, match_idx)
        res.middle_hit_reads = n_split
        if consensing:
            lap("plan_output")
            try:
                quality_kw = {}
                if umi_consensus_fastq is not None:
                    from . import consensus as cs
                    quality_kw = dict(fastq=umi_consensus_fastq,
                                      qual_table=cs.quality_table(int(umi_consensus_vote_err_pct), int(umi_consensus_max_qual)))
                res.consensus = _consensus(umi_consensus, umi_consensus_report, res, rs, reads, pr, num, pl, consensus_values,
                                           bool(umi_strands), **quality_kw)
            except Exception:                                    # nothing of this run is left behind
                for path in (umi_report, umi_groups, report):
                    if path is not None and os.path.isfile(path):
                        os.remove(path)
                raise
            lap("umi_consensus")

        lap("plan_output")
        # ---- write -------------------------------------------------------------------------
        fastq = fmt != "fasta"                                      # porechop.py:667,711,727
        if barcode_dir is not None:
            os.makedirs(barcode_dir, exist_ok=True)
        target = output if output is not None else "-"
        _, pf, paths = _piece_files([sc.calls[r] for r in pr.tolist()] if barcode_dir is not None else None, pr.size, barcode_dir,
                                    target, fmt, gz)
        file_pos = np.zeros(len(paths), dtype=np.int64)
        if pr.size:
            _emit(rs, pr, ps_, pn_, num, pf, paths, fastq, file_pos, gz)
        if barcode_dir is not None or output is not None:
            _finish_files(paths, gz, file_pos)
            res.files.update(zip(paths, map(tuple, _tally(pr, pn_, pf, len(paths), read_bases).tolist())))
        lap("write")
        return res
    finally:
        if aligner is None:
            pl.close()
        rs.close()
