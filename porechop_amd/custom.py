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
  --umi_report PATH  (with --umi) one TSV row per extracted UMI, in input order.
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
    run_cli(a, adapter_panel=panel, wildcards=a.wildcards, **kw)


if __name__ == "__main__":
    main()
