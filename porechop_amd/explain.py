"""`python -m porechop_amd.explain -i reads.fastq -o trimmed.fastq --report reads.tsv` -- the command line of
`python -m porechop_amd` (the reference's option set, unchanged there) plus --report PATH: the same run, and one TSV row per
read saying WHICH alignments decided its trims and its barcode call (runner.REPORT_COLUMNS).
--report_paths appends the alignments themselves, as run-length paths."""
from .__main__ import build_parser, run_cli


def main(argv=None):
    p = build_parser(prog="porechop_amd.explain")
    p.add_argument("--report", required=True, help="per-read explain report (TSV), written in input order")
    p.add_argument("--report_paths", action="store_true",
                   help="append start_cigars / end_cigars: the path of every listed end alignment as read_first|adapter_first|CIGAR")
    a = p.parse_args(argv)
    run_cli(a, report=a.report, report_paths=a.report_paths)


if __name__ == "__main__":
    main()
