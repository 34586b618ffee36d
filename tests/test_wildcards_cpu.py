"""IUPAC wildcards in adapters, without a GPU: the reference restatement (tests/wild_ref.py) against the committed goldens; the
one copy of the rule (pc_letters.h through pc_letter_set); the two plain-int32 routines with the adapter as sets, host-compiled
under ASan and UBSan, against wild_ref; the prefilter plan's Eq words and seedability in both modes; the runner over a
wild_ref-backed stand-in aligner; and the command line of python -m porechop_amd.custom."""
import os
import subprocess
import sys

import pytest

from tests import golden_io, wild_ref, wild_runner_case, wildgen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CSRC = os.path.join(REPO, "porechop_amd", "csrc")


def test_wild_ref_reproduces_the_goldens_for_adapters_of_bases():
    """Consequence (i): an adapter of A/C/G/T/U alone gives the same records with wildcards on.  Every 7th of the goldens with
    such a (non-empty) adapter, in wildcard mode, must reproduce the recorded reference string exactly."""
    cases = [c for c in golden_io.load_synthetic() if c[1] and not set(c[1].upper()) - set("ACGTU")]
    assert len(cases) == 15301
    sample = cases[::7]
    assert len(sample) == 2186
    assert sum(1 for c in sample if set(c[0].upper()) - set("ACGTU")) > 300          # read N / '-' among them
    assert any(set(c[0]) & set("acgt") for c in sample) and any(c[2][2] == c[2][3] for c in sample)      # lower case, linear schemes
    assert max(len(c[1]) for c in sample) >= 100 and max(len(c[0]) for c in sample) >= 300
    rec, _ = wild_ref.align_many([(c[0], c[1]) for c in sample], [c[2] for c in sample], wildcards=True)
    bad = [(c, wild_ref.format_record(r)) for c, r in zip(sample, rec)
           if golden_io.comparable(wild_ref.format_record(r)) != golden_io.comparable(c[3])]
    assert not bad, bad[:3]


def test_wild_ref_without_wildcards_is_the_reference_on_every_adapter():
    """The other mode, over adapters with N and junk as well: every 23rd golden case."""
    sample = golden_io.load_synthetic()[::23]
    rec, _ = wild_ref.align_many([(c[0], c[1]) for c in sample], [c[2] for c in sample], wildcards=False)
    bad = [(c, wild_ref.format_record(r)) for c, r in zip(sample, rec)
           if golden_io.comparable(wild_ref.format_record(r)) != golden_io.comparable(c[3])]
    assert not bad, bad[:3]


def test_the_two_consequences_in_the_reference():
    rec, paths = wild_ref.align_many([("NNNN", "NNNN")] * 2, wildcards=False)
    assert paths[0][2] == "4=" and rec[0][4] == 12
    rec, paths = wild_ref.align_many([("NNNN", "NNNN"), ("ACGT", "NNNN"), ("AC-T", "NNNN")], wildcards=True)
    assert rec[0][5] == 0 and "=" not in paths[0][2]            # an unknown read base matches nothing, not even N
    assert paths[1][2] == "4=" and rec[1][4] == 12
    assert rec[2][5] < 4


def test_letter_table_through_the_library():
    """pc_letters.h, the whole table in both modes, both cases, U, junk bytes -- stated here letter by letter."""
    from porechop_amd.batch import letter_set
    A, C, G, T, OTHER = 1, 2, 4, 8, 16
    table = {"A": A, "C": C, "G": G, "T": T, "U": T, "R": A | G, "Y": C | T, "S": C | G, "W": A | T, "K": G | T, "M": A | C,
             "B": C | G | T, "D": A | G | T, "H": A | C | T, "V": A | C | G, "N": A | C | G | T}
    for ch, want in table.items():
        for c in (ch, ch.lower()):
            assert letter_set(c, True) == want, c
            assert letter_set(c, False) == (want if ch in "ACGTU" else OTHER), c
    for b in range(256):
        if chr(b).upper() not in table:
            assert letter_set(b, True) == 0 and letter_set(b, False) == OTHER, b
        assert letter_set(b, True) & OTHER == 0
        assert letter_set(b, True) == wild_ref.letter_set(b, True) and letter_set(b, False) == wild_ref.letter_set(b, False)
    from porechop_amd._lib import load_library
    assert load_library().pc_letter_set(-1, 1) == 0 and load_library().pc_letter_set(256, 0) == 0


def _dump(cases, path):
    lines = []
    for wc in (True, False):
        ks = [k for k, c in enumerate(cases) if c[3] == wc]
        rec, paths = wild_ref.align_many([(cases[k][0], cases[k][1]) for k in ks], [cases[k][2] for k in ks], wildcards=wc)
        for k, r, p in zip(ks, rec, paths):
            rd, ad, sc, _ = cases[k]
            lines.append("%s %s %d %d %d %d %d  %s  %d %d %s" % (rd or ".", ad or ".", sc[0], sc[1], sc[2], sc[3], int(wc),
                                                                  " ".join(str(int(x)) for x in r), p[0], p[1], p[2] or "."))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def test_plain_int32_routines_with_sets_on_the_host(tmp_path):
    """pcs::align_pair_sets and pcpath::align_path_window_sets (tests/host/test_wildcards.cpp, ASan + UBSan, a stand-alone
    program) against 1500 cases dumped from wild_ref: records, path heads and run-length strings."""
    cases = wildgen.host_cases()
    _dump(cases, str(tmp_path / "cases.txt"))
    exe = str(tmp_path / "test_wildcards")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", CSRC, os.path.join(REPO, "tests", "host", "test_wildcards.cpp"),
                           "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    count = {k: int(out.stdout.split(k + "=")[1].split()[0]) for k in ("cases", "bad", "wildcards", "degenerate", "gapped", "linear")}
    assert count["cases"] == len(cases) and count["bad"] == 0
    assert count["degenerate"] > 500 and count["gapped"] > 200 and count["linear"] > 200 and count["wildcards"] < count["cases"]


def test_prefilter_plan_eq_words_and_seeds_in_both_modes(tmp_path):
    """pc_prefilter_plan.h on the host (tests/host/test_wildcards_plan.cpp): with wildcards on a row's Eq bit is set for exactly
    the bases of its set, on every route; a piece with a degenerate letter has no seeds; off, the words are the Dna5 equality's
    (and the plane's match-all rows for non-bases)."""
    exe = str(tmp_path / "test_wildcards_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", CSRC, os.path.join(REPO, "tests", "host", "test_wildcards_plan.cpp"),
                           "-o", exe])
    plain = "AATGTACTTCGTTCAGTTACGTATTGCT"
    adapters = [(wildgen.UMI28, 3), (wildgen.PRIMER22, 2), (plain, 3), ("ACGTRYSWKMBDHVNX-acgtn", 2), (wildgen.SPACER31, 3)]
    out = subprocess.run([exe] + [str(x) for ad in adapters for x in ad], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.strip().split("\n")]
    assert len(rows) == len(adapters) * 6
    seen_seeded = set()
    for f in rows:
        ad, route, mode, seeded, seeds_only, ln = f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5])
        eq = [int(x, 16) for x in f[6:11]]
        table = [int(x, 16) for x in f[11:]]
        assert ln == min(len(ad), 32) and len(table) == (4 if route == 2 else 256)
        below = 0xFFFFFFFF >> ln if ln < 32 else 0
        for code in range(5):
            want = below
            for r in range(ln):
                if wild_ref.letter_set(ord(ad[r]), bool(mode)) >> code & 1:
                    want |= 1 << (32 - ln + r)
            assert eq[code] == want, (ad, route, mode, code)
        if mode:
            assert eq[4] == below                                  # an unknown read base matches no row
        for k, word in enumerate(table):
            if route == 2:
                # over the plane a read's non-base reads as A; off, a non-base adapter letter matches all four codes
                assert word == eq[k] | (0 if mode else eq[4] & ~below), (ad, mode, k)
            else:
                assert word == eq[wild_ref.read_code(k)], (ad, route, mode, k)
        degenerate = any(wild_ref.letter_set(ord(c), True) != wild_ref.letter_set(ord(c), False) for c in ad[:ln])
        if degenerate and (mode or route):
            assert seeded == 0 and seeds_only == 0, (ad, route, mode)
        if seeded:
            seen_seeded.add((ad, route, mode))
    # adapters of bases alone are seeded as ever, in both modes and on every route
    assert {(plain, r, m) for r in range(3) for m in range(2)} <= seen_seeded


def _run(tmp_path, tag, wildcards, **kw):
    from porechop_amd import runner
    from tests.wild_aligner import WildAligner
    reads, expected = wild_runner_case.build()
    inp = wild_runner_case.write_fastq(tmp_path / "reads.fastq", reads)
    out = str(tmp_path / ("out_%s.fastq" % tag))
    res = runner.run(inp, output=out, aligner=WildAligner(), adapter_panel=wild_runner_case.adapter_sets(),
                     wildcards=wildcards, **kw)
    return reads, expected, wild_runner_case.read_fastq(out), res


def test_runner_trims_and_splits_umi_adapters_with_wildcards(tmp_path):
    reads, expected, got, res = _run(tmp_path, "on", True)
    assert res.matching_sets == ["UMI kit"]
    assert [s for _, s in got] == [p for pieces in expected for p in pieces]
    assert [n for n, _ in got][-2:] == ["read_41_1", "read_41_2"]
    assert (res.start_trim == 30).all() and (res.end_trim == 24).all()


def test_runner_leaves_the_same_reads_untrimmed_without_wildcards(tmp_path):
    reads, _, got, res = _run(tmp_path, "off", False)
    assert res.matching_sets == []
    assert [s for _, s in got] == reads
    assert not res.start_trim.any() and not res.end_trim.any()


def test_custom_command_line(tmp_path, capsys):
    from porechop_amd import custom
    from porechop_amd.panel import load_panel
    fa = tmp_path / "mine.fasta"
    fa.write_text(">UMI kit_start\n%s\n>UMI kit_end\n%s\n" % (wildgen.UMI28.lower(), wildgen.PRIMER22))
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq", "--adapters", str(fa), "--wildcards", "--only_custom",
                                                 "--report", "r.tsv", "--report_paths", "--report_middle_paths"])
    assert a.wildcards and a.only_custom and a.report == "r.tsv" and a.report_paths and a.report_middle_paths and a.end_size == 150
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq"])
    assert not a.wildcards and not a.only_custom and a.adapters is None and a.report is None
    only = custom.custom_panel(str(fa), True)
    assert [(s.name, s.start, s.end) for s in only] == [("UMI kit", ("UMI kit_start", wildgen.UMI28), ("UMI kit_end", wildgen.PRIMER22))]
    both = custom.custom_panel(str(fa), False)
    assert len(both) == len(load_panel()) + 1 and both[-1].name == "UMI kit"
    assert custom.custom_panel(None, False) is None
    # FASTA errors end the program with the message, before anything runs
    bad = tmp_path / "bad.fasta"
    for text, word in ((">kit\nACGT\n", "_start or"), ("ACGT\n", "FASTA header"), (">k_start\n\n", "no sequence"),
                       (">k_start\nAC\n>k_start\nAC\n", "twice"), ("", "no adapter record")):
        bad.write_text(text)
        with pytest.raises(SystemExit) as e:
            custom.main(["-i", "x.fastq", "--adapters", str(bad)])
        assert word in str(e.value), (text, e.value)
    for argv, word in ((["-i", "x.fastq", "--adapters", str(tmp_path / "missing.fasta")], "cannot read"),
                       (["-i", "x.fastq", "--only_custom"], "needs --adapters")):
        with pytest.raises(SystemExit) as e:
            custom.main(argv)
        assert word in str(e.value)
    # a set named like a built-in one is refused rather than silently shadowed
    bad.write_text(">%s_start\nACGTACGTACGT\n" % load_panel()[0].name)
    with pytest.raises(SystemExit) as e:
        custom.main(["-i", "x.fastq", "--adapters", str(bad)])
    assert "already in the built-in panel" in str(e.value)


def test_the_options_stay_the_references():
    """wildcards is a keyword of run(), not an Option: the parser of python -m porechop_amd is pinned to the reference's."""
    from porechop_amd import runner
    assert "wildcards" not in runner.Options.__dataclass_fields__
    p = subprocess.run([sys.executable, "-m", "porechop_amd", "-i", "x.fastq", "--wildcards"], capture_output=True, text=True, cwd=REPO)
    assert p.returncode != 0 and "unrecognized arguments" in p.stderr
