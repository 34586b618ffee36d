#!/usr/bin/env python3
"""Mint tests/golden/explain_goldens.json.gz from the REFERENCE ITSELF: what its NanoporeRead objects hold about WHY each
read was trimmed and called, for some of the whole-run cases of tests/readgen.py.

Run in the build container (needs the reference checkout and g++):

    python tests/golden/make_explain_golden.py

The reference is staged outside the repository exactly as tests/golden/make_golden.py stages it and imported from there, at
mint time only.  For every case this drives porechop/porechop.py's OWN phase functions in main()'s order --
find_matching_adapter_sets (:286-327) and the set-level rules, find_adapters_at_read_ends (:438-514),
find_adapters_in_read_middles (:533-595) -- over the seeded dataset, then dumps per read
  start_adapter_alignments / end_adapter_alignments   (set name, full identity, aligned identity, read_start, read_end)
  start_trim_amount / end_trim_amount
  best / second-best start and end barcode, barcode_call, albacore_barcode_call
  the middle hits of middle_hit_str                   (adapter name, read_start, read_end, the printed identity)
Data the reference computes while it runs; none of its program text is copied."""
import gzip
import io
import json
import os
import re
import shutil
import sys
import tempfile
from contextlib import redirect_stderr, redirect_stdout

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_golden import stage_reference  # noqa: E402
from tests import readgen  # noqa: E402

# cases of readgen.RUNNER_CASES: without barcodes (ligation reads with chimeric junctions: middle hits), a barcode run,
# --require_two_barcodes, native reads without binning (two sets at one end, junctions), an Albacore directory (the
# agreement rule), and -- GPU test only, like the case itself -- every threshold loose
CASES = ["ligation_default", "native_default", "native_bins", "native_bins_two", "albacore_bins", "native_loose"]
OUT = os.path.join(HERE, "explain_goldens.json.gz")

MIDDLE_LINE = re.compile(r"^  (.*) \(read coords: (-?\d+)-(-?\d+), identity: ([0-9.]+)%\)$")


def mint_case(pp, adapters_mod, name, dataset, mode, extra, tmp):
    inp = readgen.build_dataset(dataset, os.path.join(tmp, "datasets_" + name))
    for a in adapters_mod.ADAPTERS:
        a.best_start_score, a.best_end_score = 0.0, 0.0
    target = os.path.join(tmp, "out_" + name)
    sys.argv = ["porechop", "-i", inp, "-v", "0", "--threads", "1"] + (["-b", target] if mode == "b" else ["-o", target + ".fastq"]) + extra
    args = pp.get_arguments()
    quiet = io.StringIO()
    with redirect_stdout(quiet), redirect_stderr(quiet):
        reads, check_reads, _ = pp.load_reads(args.input, args.verbosity, args.print_dest, args.check_reads)
        sets = pp.find_matching_adapter_sets(check_reads, args.verbosity, args.end_size, args.scoring_scheme_vals, args.print_dest,
                                             args.adapter_threshold, args.threads)
        sets = pp.fix_up_1d2_sets(sets)
        orientation = pp.choose_barcoding_kit(sets, args.verbosity, args.print_dest) if args.barcode_dir else None
        sets = pp.add_full_barcode_adapter_sets(sets)
        if sets:
            pp.find_adapters_at_read_ends(reads, sets, args.verbosity, args.end_size, args.extra_end_trim, args.end_threshold,
                                          args.scoring_scheme_vals, args.print_dest, args.min_trim_size, args.threads,
                                          args.barcode_dir is not None, args.barcode_threshold, args.barcode_diff,
                                          args.require_two_barcodes, orientation)
            if not args.no_split:
                pp.find_adapters_in_read_middles(reads, sets, args.verbosity, args.middle_threshold, args.extra_middle_trim_good_side,
                                                 args.extra_middle_trim_bad_side, args.scoring_scheme_vals, args.print_dest,
                                                 args.threads, args.discard_middle)
    out = []
    for rd in reads:
        middle = []
        for line in rd.middle_hit_str.split("\n"):
            if line:
                m = MIDDLE_LINE.match(line)
                middle.append([m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)])
        tup = lambda xs: [[a[0].name, a[1], a[2], a[3], a[4]] for a in xs]
        out.append({"name": rd.name, "start_trim": rd.start_trim_amount, "end_trim": rd.end_trim_amount,
                    "start": tup(rd.start_adapter_alignments), "end": tup(rd.end_adapter_alignments),
                    "best_start": list(rd.best_start_barcode), "second_start": list(rd.second_best_start_barcode),
                    "best_end": list(rd.best_end_barcode), "second_end": list(rd.second_best_end_barcode),
                    "call": rd.barcode_call, "albacore": rd.albacore_barcode_call, "middle": middle})
    return {"dataset": dataset, "mode": mode, "argv": extra, "input_sha1": readgen.dataset_sha1(inp),
            "demultiplexed": args.barcode_dir is not None, "reads": out}


def coverage(cases):
    """What the fixture must hold to be worth comparing with (the test asserts the same)."""
    reads = [r for c in cases.values() for r in c["reads"]]
    demux = [r for c in cases.values() if c["demultiplexed"] for r in c["reads"]]
    return {"two_alignments_on_one_side": any(len(r["start"]) >= 2 or len(r["end"]) >= 2 for r in reads),
            "no_alignment": any(not r["start"] and not r["end"] for r in reads),
            "called": any(r["call"] != "none" for r in demux),
            "none": any(r["call"] == "none" for r in demux),
            "two_middle_hits": any(len(r["middle"]) >= 2 for r in reads)}


def main():
    tmp = tempfile.mkdtemp(prefix="pc_explain_golden_")
    try:
        refdir = stage_reference(tmp)
        sys.path.insert(0, refdir)
        import porechop.adapters as adapters_mod          # the reference's modules, unchanged
        import porechop.porechop as pp
        table = {c[0]: c for c in readgen.RUNNER_CASES}
        cases = {}
        for name in CASES:
            cases[name] = mint_case(pp, adapters_mod, *table[name], tmp)
            print("  case %-20s reads=%d alignments=%d middle=%d" % (
                name, len(cases[name]["reads"]), sum(len(r["start"]) + len(r["end"]) for r in cases[name]["reads"]),
                sum(len(r["middle"]) for r in cases[name]["reads"])))
        cov = coverage(cases)
        assert all(cov.values()), cov
        with gzip.GzipFile(OUT, "wb", compresslevel=9, mtime=0) as f:
            f.write(json.dumps({"generator": "tests/golden/make_explain_golden.py", "cases": cases}, sort_keys=True).encode())
        print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
