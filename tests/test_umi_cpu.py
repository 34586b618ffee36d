"""UMI extraction without a GPU: the rule on hand-stated cases (tests/umi_ref.py over tests/wild_ref.py's paths),
pc_readset_annotate through every writer (host code), the runner's UMI route on the stand-in of tests/umi_aligner.py with the
output stated byte for byte (tests/umi_runner_case.py), every refusal and the command line's two options."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import umi_ref, umi_runner_case, wild_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the rule, on cases stated by hand -------------------------------------------------------------------------------------
PREFIX, UMI28, SUFFIX = "CAAGCAGAAGACGGCATACGAGAT", "TTTVVVVTTVVVVTTVVVVTTVVVVTTT", "GTGACTGGAGTTCAG"
ADAPTER = PREFIX + UMI28 + SUFFIX                  # 67 rows; the span is rows 24 + 3 .. 24 + 24
INSTANCE = "TTTACGATTGCAATTCGCATTAACGTTT"
LEAD = "GTCTGA"                                    # six bases before the adapter's copy


def test_span_of_the_adapter():
    assert umi_ref.span(ADAPTER) == (27, 48) and umi_ref.span(UMI28) == (3, 24)
    assert umi_ref.span(PREFIX) is None and umi_ref.span(ADAPTER, wildcards=False) is None
    assert umi_ref.span("ACGNT") == (3, 3) and umi_ref.span("RACGTACY") == (0, 7) and umi_ref.span("N") == (0, 0)


HAND = [
    # (window, path the reference gives, (first, length, covered, status))
    ("exact", LEAD + PREFIX + INSTANCE + SUFFIX, (6, 0, "67="), (33, 22, 22, 0)),
    # a T under a V row (instance offset 5): a diagonal step that does not match still consumes its column under the span
    ("substitution", LEAD + PREFIX + INSTANCE[:5] + "T" + INSTANCE[6:] + SUFFIX, (6, 0, "29=1X37="), (33, 22, 22, 0)),
    # a G inserted at instance offset 10, behind the G of offset 9: the gap settles on the first of the two, before row 33 --
    # a span row behind it (27 .. 32) and one ahead: the column counts, 23 columns over 22 rows
    ("insertion", LEAD + PREFIX + INSTANCE[:10] + "G" + INSTANCE[10:] + SUFFIX, (6, 0, "33=1I34="), (33, 23, 22, 0)),
    # the C of offset 10 deleted: row 33 has no column, 21 columns over 22 rows
    ("deletion", LEAD + PREFIX + INSTANCE[:10] + INSTANCE[11:] + SUFFIX, (6, 0, "33=1D33="), (33, 21, 21, 0)),
    # the window starts at instance offset 12: the path starts at row 36, inside the span -- rows 36 .. 48 have columns 0 .. 12
    ("clipped", INSTANCE[12:] + SUFFIX, (0, 36, "31="), (0, 13, 13, 3)),
]


@pytest.mark.parametrize("name,window,path,want", HAND, ids=[h[0] for h in HAND])
def test_hand_stated_cases(name, window, path, want):
    rec, got_path = wild_ref.align(window, ADAPTER, (3, -6, -5, -2))
    assert tuple(got_path) == path
    sp = umi_ref.span(ADAPTER)
    first, length, covered, complete = umi_ref.extract(got_path, sp)
    status = umi_ref.classify(rec, got_path, sp)[0]
    assert (first, length, covered, status) == want and complete == (status == 0)
    # the bases themselves
    if name == "exact":
        assert window[first:first + length] == INSTANCE[3:25]
    if name == "insertion":
        assert window[first:first + length] == INSTANCE[3:10] + "G" + INSTANCE[10:25]


def test_edges_of_the_span_and_the_rule():
    sp = (3, 5)
    # insertions at either edge are outside: before row 3 (nothing of the span behind it) and before row 6 (nothing ahead)
    assert umi_ref.extract((10, 0, "3=1I3=2="), sp) == (14, 3, 3, True)
    assert umi_ref.extract((10, 0, "6=1I2="), sp) == (13, 3, 3, True)
    assert umi_ref.extract((10, 0, "4=1I4="), sp) == (13, 4, 3, True)
    # the whole span deleted: complete, and nothing under it
    assert umi_ref.extract((10, 0, "3=3D2="), sp) == (-1, 0, 0, True)
    # the path ends inside the span / starts inside it
    assert umi_ref.extract((10, 0, "5="), sp) == (13, 2, 2, False)
    assert umi_ref.extract((0, 4, "4="), sp) == (0, 2, 2, False)
    rule = (150, 4, 2, 75.0)
    assert umi_ref.qualifies((0, 27, 0, 27, 84, 28, 28, 28), 0, rule) and not umi_ref.qualifies((0, 27, 0, 27, 84, 28, 28, 28), 1, rule)
    assert not umi_ref.qualifies((122, 149, 0, 27, 84, 28, 28, 28), 0, rule) and umi_ref.qualifies((122, 149, 0, 27, 84, 28, 28, 28), 1, rule)
    assert not umi_ref.qualifies((5, 7, 0, 2, 9, 3, 3, 28), 0, rule) and not umi_ref.qualifies((5, 32, 0, 27, 30, 21, 28, 28), 0, rule)
    assert umi_ref.classify((-1, 0, -1, 0, -2**31, 0, 0, 0), (0, 0, ""), sp) == (1, -1, 0, 0)
    assert umi_ref.classify((5, 7, 0, 2, 9, 3, 3, 28), (5, 0, "3="), sp, 0, rule) == (2, -1, 0, 0)


# ---- pc_readset_annotate through every writer --------------------------------------------------------------------------------
READS = [("r1", "ACGTACGTAC", "IIIIIHHHHH"), ("r2 ch=7 mux=1", "GGGGCCCCAA", "5555566666"), ("r3", "TTTTTTTT", "ABCDEFGH")]


def _load(tmp_path, fastq=True, gz=False):
    from porechop_amd.io import ReadSet
    text = "".join(("@%s\n%s\n+\n%s\n" % r) if fastq else (">%s\n%s\n" % r[:2]) for r in READS)
    path = tmp_path / ("in.%s%s" % ("fastq" if fastq else "fasta", ".gz" if gz else ""))
    path.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    return ReadSet(str(path))


# pieces: r1 whole; r2 as pieces 1 and 2; r3 whole
PIECES = dict(piece_read=[0, 1, 1, 2], piece_start=[0, 0, 6, 0], piece_len=[10, 4, 4, 8], piece_number=[0, 1, 2, 0], piece_file=[0, 0, 0, 0])
TAGGED_FASTQ = ("@r1 UMI_start=ACG\nACGTACGTAC\n+\nIIIIIHHHHH\n"
                "@r2_1 ch=7 mux=1 UMI_start=TTT UMI_end=GG\nGGGG\n+\n5555\n"
                "@r2_2 ch=7 mux=1 UMI_start=TTT UMI_end=GG\nCCAA\n+\n6666\n"
                "@r3\nTTTTTTTT\n+\nABCDEFGH\n")
TAGGED_FASTA = (">r1 UMI_start=ACG\nACGTACGTAC\n>r2_1 ch=7 mux=1 UMI_start=TTT UMI_end=GG\nGGGG\n"
                ">r2_2 ch=7 mux=1 UMI_start=TTT UMI_end=GG\nCCAA\n>r3\nTTTTTTTT\n")


def _annotate(rs):
    rs.annotate([1, 0, 1], ["UMI_start=TTT", "UMI_start=ACG", "UMI_end=GG"])       # r2 is named twice: both texts, in order
    assert [rs.name(i) for i in range(3)] == ["r1 UMI_start=ACG", "r2 ch=7 mux=1 UMI_start=TTT UMI_end=GG", "r3"]


@pytest.mark.parametrize("gz_in", [False, True])
@pytest.mark.parametrize("fastq", [True, False])
def test_annotate_through_every_writer(tmp_path, fastq, gz_in):
    from porechop_amd.io import gz_finish
    rs = _load(tmp_path, fastq, gz_in)
    try:
        _annotate(rs)
        want = (TAGGED_FASTQ if fastq else TAGGED_FASTA).encode()
        p = {k: np.array(v) for k, v in PIECES.items()}
        args = (p["piece_read"], p["piece_start"], p["piece_len"], p["piece_number"], p["piece_file"])
        # write
        out = tmp_path / "w.out"
        assert rs.write(*args, [str(out)], fastq) == len(want)
        assert out.read_bytes() == want
        # write_sizes says what is written
        assert rs.write_sizes(*args, 1, fastq).tolist() == [len(want)]
        # write_at in two blocks, and write_shared behind a first block
        for second in (rs.write_at, rs.write_shared):
            out = tmp_path / ("at_%s.out" % second.__name__)
            pos = np.zeros(1, dtype=np.int64)
            rs.write_at(*(a[:2] for a in args), [str(out)], fastq, pos)
            second(*(a[2:] for a in args), [str(out)], fastq, pos)
            assert int(pos[0]) == len(want) and out.read_bytes() == want
        # compress: the .gz output of a run
        out = tmp_path / "c.out.gz"
        img = rs.compress(*args, 1, fastq)
        try:
            assert int(img.sizes()[1][0]) == len(want)
            pos = np.zeros(1, dtype=np.int64)
            img.write([str(out)], pos)
        finally:
            img.close()
        gz_finish(str(out))
        assert gzip.decompress(out.read_bytes()) == want
    finally:
        rs.close()


def test_annotate_refusals_change_nothing(tmp_path):
    rs = _load(tmp_path)
    try:
        before = [rs.name(i) for i in range(3)]
        for reads, texts in (([3], ["x"]), ([-1], ["x"]), ([0, 5], ["fine", "x"]), ([0], [""]), ([0, 1], ["fine", "a\nb"]), ([0], ["a\rb"]),
                             ([0], ["a\0b"]), ([0, 1], ["x"])):
            with pytest.raises(ValueError):
                rs.annotate(reads, texts)
            assert [rs.name(i) for i in range(3)] == before
        rs.annotate([], [])
        assert [rs.name(i) for i in range(3)] == before
        _annotate(rs)
        rs.annotate([2], ["again"])                                  # a second call appends behind the first one's texts
        rs.annotate([1], ["and again"])
        assert [rs.name(i) for i in range(3)] == ["r1 UMI_start=ACG", "r2 ch=7 mux=1 UMI_start=TTT UMI_end=GG and again", "r3 again"]
    finally:
        rs.close()


# ---- the runner on the stand-in ----------------------------------------------------------------------------------------------
def _run(tmp_path, tag, streamed=None, **kw):
    from porechop_amd import runner
    from tests.umi_aligner import UmiAligner
    reads, out_records, rows = umi_runner_case.build()
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(reads))
    out = tmp_path / ("out_%s.fastq" % tag)
    opts = runner.Options()
    opts.check_reads = 3
    common = dict(aligner=UmiAligner(), adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, **kw)
    if streamed:
        res = runner.run_streamed(str(inp), str(out), None, opts, block_bytes=streamed, **common)
        assert res is not None, "not streamed"
    else:
        res = runner.run(str(inp), output=str(out), options=opts, **common)
    return res, out.read_text(), out_records, rows


def test_runner_tags_the_reads_and_writes_the_report(tmp_path):
    report = tmp_path / "umis.tsv"
    res, text, out_records, rows = _run(tmp_path, "umi", umi=True, umi_report=str(report))
    assert res.matching_sets == [umi_runner_case.KIT]
    assert text == umi_runner_case.fastq_text(out_records)
    assert report.read_text() == umi_runner_case.report_text(rows)
    assert len(res.umis) == 12 and res.umis[7] == (None, None) and res.umis[9] == (None, None)
    assert res.umis[0] == ((umi_runner_case.KIT, 27, 22, 22, "ACGATTCGACTTGACGTTACGA"), (umi_runner_case.KIT, 67 + 240 + 12, 8, 8, "ACGTACGT"))
    assert res.umis[2][0][1:4] == (27, 23, 22) and res.umis[2][1][4] == "NACGTTGA"
    assert res.umis[3][1] is None and res.umis[5][0] is None


@pytest.mark.parametrize("block", [1500, 4000])
def test_streamed_run_writes_the_same_bytes(tmp_path, block):
    report = tmp_path / "umis_streamed.tsv"
    res, text, out_records, rows = _run(tmp_path, "streamed", streamed=block, umi=True, umi_report=str(report))
    assert text == umi_runner_case.fastq_text(out_records)
    assert report.read_text() == umi_runner_case.report_text(rows)
    whole = _run(tmp_path, "whole", umi=True)[0]
    assert res.umis == whole.umis and res.n_reads == 12


def test_without_umi_nothing_changes(tmp_path):
    res_off, text_off, out_records, _ = _run(tmp_path, "off", umi=False)
    res_plain, text_plain, _, _ = _run(tmp_path, "plain")
    assert text_off == text_plain and res_off.umis is None and res_plain.umis is None
    # the same pieces as with umi=True, under the input's own headers
    plain_headers = ["read_%d" % k for k in range(1, 11)] + ["read_11 runid=7 ch=12", "read_12_1 ch=5", "read_12_2 ch=5"]
    assert text_off == umi_runner_case.fastq_text([(h, s) for h, (_, s) in zip(plain_headers, out_records)])


# ---- refusals and the command line -------------------------------------------------------------------------------------------
def test_usage_errors(tmp_path, monkeypatch):
    from porechop_amd import runner
    from porechop_amd.pipeline import AdapterSet
    from tests.umi_aligner import UmiAligner
    reads, _, _ = umi_runner_case.build()
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(reads))
    out = str(tmp_path / "out.fastq")
    panel = umi_runner_case.adapter_sets()
    with pytest.raises(runner.UsageError, match="--umi needs --wildcards"):
        runner.run(str(inp), output=out, aligner=UmiAligner(), adapter_panel=panel, umi=True)
    with pytest.raises(runner.UsageError, match="--umi_report needs --umi"):
        runner.run(str(inp), output=out, aligner=UmiAligner(), adapter_panel=panel, wildcards=True, umi_report=str(tmp_path / "u.tsv"))
    fixed = [AdapterSet("plain kit", ("p_start", "AATGTACTTCGTTCAGTTACGTATTGCT"), ("p_end", "GCAATACGTAACTGAACGAAGT"))]
    with pytest.raises(runner.UsageError, match="degenerate letters"):
        runner.run(str(inp), output=out, aligner=UmiAligner(), adapter_panel=fixed, wildcards=True, umi=True)
    with pytest.raises(runner.UsageError, match="degenerate letters"):
        runner.run_streamed(str(inp), out, None, runner.Options(), aligner=UmiAligner(), adapter_panel=fixed, wildcards=True, umi=True,
                            block_bytes=1500)
    assert not os.path.exists(out) and not (tmp_path / "u.tsv").exists()
    # a sharded run: refused like the per-read report
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(runner.UsageError, match="sharded"):
        runner.run(str(inp), output=out, aligner=UmiAligner(), adapter_panel=panel, wildcards=True, umi=True)
    assert "umi" not in runner.Options.__dataclass_fields__


def test_command_line_options(tmp_path):
    from porechop_amd import custom
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq", "--wildcards", "--umi", "--umi_report", "u.tsv"])
    assert a.umi and a.umi_report == "u.tsv" and a.wildcards
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq"])
    assert not a.umi and a.umi_report is None
    fa = tmp_path / "umi.fasta"
    fa.write_text(">UMI kit_start\n%s\n>UMI kit_end\n%s\n" % (umi_runner_case.START, umi_runner_case.END))
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(umi_runner_case.build()[0]))
    for argv, word in ((["--umi"], "--umi needs --wildcards"), (["--wildcards", "--umi_report", "u.tsv"], "--umi_report needs --umi")):
        with pytest.raises(SystemExit) as e:
            custom.main(["-i", str(inp), "-o", str(tmp_path / "o.fastq"), "--adapters", str(fa), "--only_custom"] + argv)
        assert word in str(e.value)
    # python -m porechop_amd keeps the reference's parser
    p = subprocess.run([sys.executable, "-m", "porechop_amd", "-i", "x.fastq", "--umi"], capture_output=True, text=True, cwd=REPO)
    assert p.returncode != 0 and "unrecognized arguments" in p.stderr
