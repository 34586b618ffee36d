"""`python -m porechop_amd.custom -i reads.fastq -o trimmed.fastq --adapters mine.fasta [--only_custom] [--wildcards] [--umi]` -- the
command line of `python -m porechop_amd` (the reference's option set, unchanged there) with a custom adapter panel:
  --adapters FASTA   adapter sets as discover.read_adapters reads them (records named <set>_start / <set>_end), added to
                     the built-in panel;
  --only_custom      the FASTA's sets alone;
  --wildcards        IUPAC letters in the panel's adapters stand for their sets of bases (R = AG ... N = ACGT; a read base
                     that is not A/C/G/T/U matches nothing): UMI adapters, degenerate primers, NNNN spacers (DESIGN.md
                     section 15);
  --umi              (with --wildcards) the read bases under an adapter's degenerate letters are kept: reads whose start or
                     end adapter has such letters get UMI_start=<bases> and / or UMI_end=<bases> at the end of their header
                     (DESIGN.md section 16);
  --umi_report PATH  (with --umi) one TSV row per extracted UMI, in input order;
  --umi_groups PATH  (with --umi) which reads come from one molecule: one TSV row per read with a UMI key -- its group, the
                     key, the reads of the key and of the group, the group's representative.  The
                     distinct keys are compared all against all on the GPU by edit distance;
                     --umi_group_by start|end|both (default: both when both adapters carry a UMI), --umi_max_dist N (2),
                     --umi_group_method directional|cluster, --umi_group_max_keys N (refuse more distinct keys than N);
  --umi_consensus PATH  (with --umi) one consensus sequence per group of reads, as FASTA: the members of a
                     group are aligned to its median-length member inside a band on the GPU, vote per column, and the call is
                     the next round's template.  --umi_consensus_report PATH (a TSV row per group), --umi_consensus_min_reads N
                     (3), --umi_consensus_max_reads N (256), --umi_consensus_band N (64), --umi_consensus_rounds N (2),
                     --umi_consensus_max_err_pct N (30), --umi_consensus_max_len N (65535).  The reads stay resident: the input
                     is not streamed.
  --umi_consensus_fastq PATH  (with --umi; alone or beside --umi_consensus) the same records as FASTQ with one quality value per
                     base: the Phred value of the base's vote margin -- its votes less those of the strongest alternative --
                     from a table built for --umi_consensus_vote_err_pct N (1..50, default 10: each vote wrong with that
                     probability, independently) and capped at --umi_consensus_max_qual N (1..93, default 60).  The report gains
                     the columns expected_errors and low_qual (bases below Q10).
  --umi_strands      (with --umi, --umi_groups or --umi_consensus, and START+END keys) both strands of a molecule are one group: a
                     read of the minus strand shows the key START+END as rc(END)+rc(START), so keys are compared as they stand
                     and mirrored, the groups TSV gains a strand column (+ / -), and the consensus piles the - reads up as
                     their reverse complements and is written in the group's + orientation (minus=<n> in its header).  List
                     the UMI adapter in both orientations, as two sets, so that minus-strand reads have UMIs at all (README).
It composes with the explain report: --report PATH, --report_paths, --report_middle_paths (porechop_amd.explain)."""
import sys

from .__main__ import build_parser, run_cli


def build_custom_parser(prog="porechop_amd.custom"):
    p = build_parser(prog=prog)
    p.add_argument("--adapters", metavar="FASTA", help="custom adapter sets: FASTA records named <set>_start / <set>_end")
    p.add_argument("--only_custom", action="store_true", help="search for the sets of --adapters only, not the built-in panel")
    p.add_argument("--wildcards", action="store_true", help="IUPAC letters in adapters stand for their sets of bases")
    p.add_argument("--umi", action="store_true", help="tag every read with the bases under its adapters' degenerate letters (needs --wildcards)")
    p.add_argument("--umi_report", metavar="PATH", help="one TSV row per extracted UMI (needs --umi)")
    p.add_argument("--umi_groups", metavar="PATH", help="one TSV row per read with a UMI key: its group of reads of one molecule (needs --umi)")
    p.add_argument("--umi_group_by", choices=["start", "end", "both"], default=None,
                   help="the UMIs that make a read's key (default: both when both adapters carry one, else the side that does)")
    p.add_argument("--umi_max_dist", type=int, default=2, help="keys within this many edits are neighbours (default: 2)")
    p.add_argument("--umi_group_method", choices=["directional", "cluster"], default="directional",
                   help="directional: a key joins a neighbour with at least 2n-1 of its n reads; cluster: connected components")
    p.add_argument("--umi_group_max_keys", type=int, default=1 << 20, help="refuse to compare more distinct keys than this (default: 1048576)")
    p.add_argument("--umi_consensus", metavar="PATH", help="one consensus sequence per UMI group, FASTA (needs --umi)")
    p.add_argument("--umi_consensus_report", metavar="PATH", help="one TSV row per UMI group: members, used, rejected, skipped, rounds, length, status")
    p.add_argument("--umi_consensus_min_reads", type=int, default=3, help="groups with fewer members get no sequence (default: 3)")
    p.add_argument("--umi_consensus_max_reads", type=int, default=256, help="only a group's first N members take part (default: 256)")
    p.add_argument("--umi_consensus_band", type=int, default=64, help="half width of the alignment band around the stretched diagonal, 1..127 (default: 64)")
    p.add_argument("--umi_consensus_rounds", type=int, default=2, help="rounds: a round's consensus is the next one's template (default: 2)")
    p.add_argument("--umi_consensus_max_err_pct", type=int, default=30, help="a member further than this from the template sits the round out (default: 30)")
    p.add_argument("--umi_consensus_max_len", type=int, default=65535, help="groups whose template is longer get no sequence (default: 65535)")
    p.add_argument("--umi_consensus_fastq", metavar="PATH", help="the consensus sequences as FASTQ, one quality value per base from its vote margin (needs --umi)")
    p.add_argument("--umi_consensus_vote_err_pct", type=int, default=None,
                   help="the quality table's model: each vote is wrong with this probability in percent, 1..50 (default: 10; needs --umi_consensus_fastq)")
    p.add_argument("--umi_consensus_max_qual", type=int, default=None, help="the highest quality value written, 1..93 (default: 60; needs --umi_consensus_fastq)")
    p.add_argument("--umi_strands", action="store_true",
                   help="group and call across both strands of a molecule: a key START+END also matches its mirror rc(END)+rc(START) "
                        "(needs --umi, --umi_groups or --umi_consensus, and keys of both sides)")
    p.add_argument("--report", help="per-read explain report (TSV), written in input order")
    p.add_argument("--report_paths", action="store_true", help="append start_cigars / end_cigars to the report")
    p.add_argument("--report_middle_paths", action="store_true", help="append middle_cigars to the report")
    return p


def custom_panel(path, only_custom):
    """The panel of a run: the FASTA's sets behind the built-in ones, or alone.  None: the built-in panel as it is."""
    from . import panel as panel_rules
    from .discover import read_adapters
    if path is None:
        if only_custom:
            raise ValueError("Error: --only_custom needs --adapters")
        return None
    try:
        sets = read_adapters(path)
    except OSError as e:
        raise ValueError("Error: cannot read %s: %s" % (path, e.strerror or e))
    if not sets:
        raise ValueError("Error: %s holds no adapter record" % path)
    if only_custom:
        return sets
    builtin = panel_rules.load_panel()
    taken = {s.name for s in builtin}
    for s in sets:
        if s.name in taken:
            raise ValueError("Error: adapter set %r of %s is already in the built-in panel" % (s.name, path))
    return builtin + sets


def main(argv=None):
    a = build_custom_parser().parse_args(argv)
    try:
        panel = custom_panel(a.adapters, a.only_custom)
    except ValueError as e:
        sys.exit(str(e))
    kw = {}
    if a.report is not None or a.report_paths or a.report_middle_paths:
        kw = dict(report=a.report, report_paths=a.report_paths, report_middle_paths=a.report_middle_paths)
    if a.umi or a.umi_report is not None:
        kw.update(umi=a.umi, umi_report=a.umi_report)
    if a.umi_groups is not None:
        kw.update(umi=a.umi, umi_groups=a.umi_groups, umi_group_by=a.umi_group_by, umi_max_dist=a.umi_max_dist,
                  umi_group_method=a.umi_group_method, umi_group_max_keys=a.umi_group_max_keys)
    if a.umi_consensus_fastq is None and (a.umi_consensus_vote_err_pct is not None or a.umi_consensus_max_qual is not None):
        sys.exit("Error: --umi_consensus_vote_err_pct and --umi_consensus_max_qual need --umi_consensus_fastq")
    if a.umi_consensus is not None or a.umi_consensus_report is not None or a.umi_consensus_fastq is not None:
        if a.umi_consensus_fastq is not None:
            kw.update(umi_consensus_fastq=a.umi_consensus_fastq,
                      umi_consensus_vote_err_pct=10 if a.umi_consensus_vote_err_pct is None else a.umi_consensus_vote_err_pct,
                      umi_consensus_max_qual=60 if a.umi_consensus_max_qual is None else a.umi_consensus_max_qual)
        kw.update(umi=a.umi, umi_consensus=a.umi_consensus, umi_consensus_report=a.umi_consensus_report,
                  umi_group_by=a.umi_group_by, umi_max_dist=a.umi_max_dist, umi_group_method=a.umi_group_method,
                  umi_group_max_keys=a.umi_group_max_keys, umi_consensus_min_reads=a.umi_consensus_min_reads,
                  umi_consensus_max_reads=a.umi_consensus_max_reads, umi_consensus_band=a.umi_consensus_band,
                  umi_consensus_rounds=a.umi_consensus_rounds, umi_consensus_max_err_pct=a.umi_consensus_max_err_pct,
                  umi_consensus_max_len=a.umi_consensus_max_len)
    if a.umi_strands:
        kw.update(umi=a.umi, umi_strands=True, umi_group_by=a.umi_group_by)
    run_cli(a, adapter_panel=panel, wildcards=a.wildcards, **kw)


if __name__ == "__main__":
    main()
