"""`python -m porechop_amd.explain -i reads.fastq -o trimmed.fastq --report reads.tsv` -- the command line of
`python -m porechop_amd` (the reference's option set, unchanged there) plus --report PATH: the same run, and one TSV row per
read saying WHICH alignments decided its trims and its barcode call (runner.REPORT_COLUMNS)."""
from .__main__ import build_parser, run_cli


def main(argv=None):
    p = build_parser(prog="porechop_amd.explain")
    p.add_argument("--report", required=True, help="per-read explain report (TSV), written in input order")
    a = p.parse_args(argv)
    run_cli(a, report=a.report)


if __name__ == "__main__":
    main()
