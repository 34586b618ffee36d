"""Shared driver of the explain golden cases (tests/golden/explain_goldens.json.gz, minted from the reference's own
NanoporeRead objects by tests/golden/make_explain_golden.py on the seeded inputs of tests/readgen.py): runs
porechop_amd.runner with report=..., compares every read's reasons with the reference's, floats with ==."""
import gzip
import json
import os

from tests import readgen
from tests.runner_cases import options_from_argv

GOLDENS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain_goldens.json.gz")
COLUMNS = 17


def load_goldens():
    with gzip.open(GOLDENS, "rt") as f:
        return json.load(f)["cases"]


def coverage(cases):
    """The fixture is not trivial: it holds each of the situations the report exists to tell apart."""
    reads = [r for c in cases.values() for r in c["reads"]]
    demux = [r for c in cases.values() if c["demultiplexed"] for r in c["reads"]]
    return {"two_alignments_on_one_side": any(len(r["start"]) >= 2 or len(r["end"]) >= 2 for r in reads),
            "no_alignment": any(not r["start"] and not r["end"] for r in reads),
            "called": any(r["call"] != "none" for r in demux),
            "none": any(r["call"] == "none" for r in demux),
            "two_middle_hits": any(len(r["middle"]) >= 2 for r in reads)}


def run_with_report(name, case, workdir, datasets, make_aligner=None, device=None, streamed_block=None):
    """-> (RunResult, report text, {output file -> md5})"""
    from porechop_amd import runner
    if case["dataset"] not in datasets:
        path = readgen.build_dataset(case["dataset"], os.path.join(workdir, "datasets"))
        assert readgen.dataset_sha1(path) == case["input_sha1"], "tests/readgen.py drifted from the goldens"
        datasets[case["dataset"]] = path
    inp = datasets[case["dataset"]]
    opts = options_from_argv(case["argv"])
    work = os.path.join(workdir, "explain_" + name + ("_streamed" if streamed_block else ""))
    os.makedirs(work)
    kw = {"device": device}
    if make_aligner is not None:
        kw["aligner"] = make_aligner(opts.scoring_scheme)
    target = os.path.join(work, "bins" if case["mode"] == "b" else case["mode"][2:])
    report = os.path.join(work, "report.tsv")
    out = {"barcode_dir": target} if case["mode"] == "b" else {"output": target}
    if streamed_block:
        res = runner.run_streamed(inp, out.get("output"), out.get("barcode_dir"), opts, block_bytes=streamed_block, report=report, **kw)
        assert res is not None, "not streamed"
    else:
        res = runner.run(inp, options=opts, report=report, **out, **kw)
    with open(report) as f:
        text = f.read()
    return res, text, readgen.output_md5s(target)


def check_against_golden(name, golden, res, text):
    """Every read: alignment lists, trims, best and second-best barcodes with scores, final call, middle hits."""
    opts = options_from_argv(golden["argv"])
    ex = res.explain
    reads = golden["reads"]
    lines = text.split("\n")
    assert lines[0].startswith("#name\tlength\tstart_trim\tend_trim\t") and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert len(rows) == len(reads) == res.n_reads == ex.summary.shape[0], (name, len(rows), len(reads))
    for r, (g, row) in enumerate(zip(reads, rows)):
        where = (name, r, g["name"])
        assert len(row) == COLUMNS and row[0] == g["name"].replace("\t", " "), where
        starts, ends = ex.end_alignments(r)
        assert [list(x) for x in starts] == g["start"], (where, starts, g["start"])
        assert [list(x) for x in ends] == g["end"], (where, ends, g["end"])
        assert (int(res.start_trim[r]), int(res.end_trim[r])) == (g["start_trim"], g["end_trim"]) == tuple(int(x) for x in ex.summary[r, 0:2]), where
        assert (int(ex.summary[r, 2]), int(ex.summary[r, 3])) == (len(g["start"]), len(g["end"])), where
        assert row[2:4] == [str(g["start_trim"]), str(g["end_trim"])], where
        fmt = lambda xs: ";".join("%s|%.6f|%.6f|%d|%d" % tuple(x) for x in xs) or "."
        assert row[4:6] == [fmt(g["start"]), fmt(g["end"])], where
        # the deciding job: the FIRST listed alignment of its side whose own trim amount is the read's trim
        # (nanopore_read.py:180-181,202-203: max() keeps the earlier of two equal amounts)
        rows = ex.hits[int(ex.hit_first[r]):int(ex.hit_first[r + 1])].tolist()
        for side in (0, 1):
            amounts = [(j, (re + opts.extra_end_trim) if side == 0 else (opts.end_size - rs) + opts.extra_end_trim)
                       for j, rs, re, _, _, _ in rows if ex.job_side[j] == side]
            trim = int(ex.summary[r, side])
            assert trim == max([0] + [t for _, t in amounts]), where
            first = next((j for j, t in amounts if t == trim), -1) if trim > 0 else -1
            assert int(ex.summary[r, 4 + side]) == first, (where, side, amounts, trim)
        mids = ex.middle_hits(r)
        assert [[m[0], m[1], m[2], "%.1f" % m[3]] for m in mids] == g["middle"], (where, mids, g["middle"])
        assert row[6] == (";".join("%s|%d|%d|%.6f" % m for m in mids) or "."), where
        if golden["demultiplexed"]:
            want = tuple((x[0], x[1]) for x in (g["best_start"], g["second_start"], g["best_end"], g["second_end"]))
            assert ex.barcodes(r) == want, (where, ex.barcodes(r), want)
            assert res.barcode_calls[r] == g["call"] == row[16], (where, res.barcode_calls[r], g["call"])
            assert row[15] == (g["albacore"] if g["albacore"] is not None else "."), where
            assert row[7:15] == [s for x in want for s in (x[0], "%.6f" % x[1])], where
        else:
            assert row[7:] == ["."] * 10, where
