"""Per-base quality values of the UMI consensus without a GPU ("Quality values"): the default table, the
vote margins of the numpy model (consensus.round_host(qual_table=...)) on hand-stated pile-ups, the qualities' way through the
rounds (call_groups), the FASTQ and the report's two columns, the runner on the stand-in aligner (the host route) and the
command line.  The GPU tests (tests/test_gpu_consensus_quality.py) compare the kernel with this model."""
import random

import numpy as np
import pytest

from porechop_amd import consensus as cs
from tests import consensus_case as ccase
from tests import umi_runner_case

# a table that shows the margin itself: entry m is m (the rule's index stops at 255, a Phred value at 93)
MARGIN = np.minimum(np.arange(256), 93).astype(np.uint8)


def margins(tmpl, members, tmpl_counts=1, band=4, pct=30):
    r = cs.round_host([tmpl], members, [0] * len(members), band, pct, tmpl_counts=tmpl_counts, qual_table=MARGIN)
    assert r.qual.dtype == np.uint8 and r.qual.shape == r.cons.shape
    return r.cons.tobytes(), r.qual.tolist()


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_the_default_table():
    t = cs.quality_table(10, 60)
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert t[:6].tolist() == [1, 10, 25, 41, 56, 60] and (t[5:] == 60).all()
    assert np.array_equal(cs.quality_table(), t)
    for eps in (1, 10, 50):
        for cap in (1, 60, 93):
            t = cs.quality_table(eps, cap)
            assert (np.diff(t.astype(np.int64)) >= 0).all() and int(t.max()) == cap and int(t[255]) == cap, (eps, cap)
    # e = 50 %: r = 4, entry m = round(10 log10(1 + 4^m / 4)): 1 + 1/4, 1 + 1, 1 + 4, 1 + 16
    assert cs.quality_table(50, 93)[:4].tolist() == [1, 3, 7, 12]
    # e = 1 %: r = 396: 10 log10(1 + 99) = 20
    assert cs.quality_table(1, 93)[:2].tolist() == [1, 20]


def test_the_tables_refusals():
    for kw in (dict(vote_err_pct=0), dict(vote_err_pct=51), dict(vote_err_pct=-1), dict(vote_err_pct=2.5), dict(max_qual=0), dict(max_qual=94)):
        with pytest.raises(ValueError):
            cs.quality_table(**kw)
    bad = MARGIN.copy()
    bad[7] = 94
    for table in (bad, MARGIN[:255], MARGIN.astype(np.float64)):
        with pytest.raises(ValueError):
            cs.round_host([b"ACGT"], [b"ACGT"], [0], 4, 30, qual_table=table)


# ---- hand-stated pile-ups ---------------------------------------------------------------------------------------------------------
def test_a_column_outvoted_three_to_one():
    # voters: the template and three members.  Column 3: A 3, the template's T 1; every other column 4 : 0
    assert margins(b"ACGTACGTAC", [b"ACGAACGTAC"] * 3) == (b"ACGAACGTAC", [4, 4, 4, 2, 4, 4, 4, 4, 4, 4])
    # the template as an earlier consensus: its vote is no evidence -- 3 : 0 everywhere
    assert margins(b"ACGTACGTAC", [b"ACGAACGTAC"] * 3, tmpl_counts=0) == (b"ACGAACGTAC", [3] * 10)
    # the default table on the same pile-up
    r = cs.round_host([b"ACGTACGTAC"], [b"ACGAACGTAC"] * 3, [0] * 3, 4, 30, qual_table=cs.quality_table())
    assert r.qual.tolist() == [56, 56, 56, 25, 56, 56, 56, 56, 56, 56]


def test_a_tie_the_template_decides():
    # members 2 : 2 in column 3; the template's T makes it 3 : 2 when it is a read of the group, and only breaks the tie when not
    members = [b"ACGACA", b"ACGACA", b"ACGTCA", b"ACGTCA"]
    assert margins(b"ACGTCA", members) == (b"ACGTCA", [5, 5, 5, 1, 5, 5])
    assert margins(b"ACGTCA", members, tmpl_counts=0) == (b"ACGTCA", [4, 4, 4, 0, 4, 4])
    # 1 : 1 with the template's vote included: a tie either way; as an earlier consensus the template's base is even behind
    assert margins(b"ACGTCA", [b"ACGACA"]) == (b"ACGTCA", [2, 2, 2, 0, 2, 2])
    assert margins(b"ACGTCA", [b"ACGACA"], tmpl_counts=0) == (b"ACGTCA", [1, 1, 1, 0, 1, 1])
    # a base against a deletion, one vote each: deletion is one of the alternatives
    assert margins(b"ACGTCA", [b"ACGCA"]) == (b"ACGTCA", [2, 2, 2, 0, 2, 2])


def test_an_insertion_held_by_three_of_four_voters():
    # slot 0 of gap 3: T 3, one voter (the template) holds nothing there: 3 - 1
    assert margins(b"ACGACA", [b"ACGTACA"] * 3) == (b"ACGTACA", [4, 4, 4, 2, 4, 4, 4])
    # the template as an earlier consensus is no voter: three of three
    assert margins(b"ACGACA", [b"ACGTACA"] * 3, tmpl_counts=0) == (b"ACGTACA", [3, 3, 3, 3, 3, 3, 3])
    # three of five: emitted (2 * 3 > 5), 3 against 2 absent
    assert margins(b"ACGACA", [b"ACGTACA", b"ACGTACA", b"ACGACA", b"ACGTACA"]) == (b"ACGTACA", [5, 5, 5, 1, 5, 5, 5])
    # the holders disagree: T 2, C 1 of four voters -- emitted (2 * 3 > 4), T leads C by one and the absent one by one.  (An
    # inserted C cannot slide into another gap here: its neighbours are G and A.)
    assert margins(b"ACGACA", [b"ACGTACA", b"ACGTACA", b"ACGCACA"]) == (b"ACGTACA", [4, 4, 4, 1, 4, 4, 4])
    # T 2, C 2 of five voters: emitted, ties to the smaller code, margin 0
    assert margins(b"ACGACA", [b"ACGTACA", b"ACGTACA", b"ACGCACA", b"ACGCACA"]) == (b"ACGCACA", [5, 5, 5, 0, 5, 5, 5])


def test_an_n_abstains():
    # column 3 holds the template's T alone: 1 : 0 as a read of the group, 0 : 0 as an earlier consensus
    assert margins(b"ACGTCA", [b"ACGNCA"] * 3) == (b"ACGTCA", [4, 4, 4, 1, 4, 4])
    assert margins(b"ACGTCA", [b"ACGNCA"] * 3, tmpl_counts=0) == (b"ACGTCA", [3, 3, 3, 0, 3, 3])
    # an N in the template: nothing is taken off for it
    assert margins(b"ACGNCA", [b"ACGCCA", b"ACGCCA"], tmpl_counts=0) == (b"ACGCCA", [2, 2, 2, 2, 2, 2])


def test_a_deleted_column_has_no_quality_and_the_clamp():
    cons, q = margins(b"ACGTCA", [b"ACGCA"] * 3)
    assert cons == b"ACGCA" and q == [4, 4, 4, 4, 4]
    # 300 members: the margin passes 255 and the table's last entry decides
    table = ((7 * np.arange(256) + 3) % 94).astype(np.uint8)
    r = cs.round_host([b"ACGT"], [b"ACGT"] * 300, [0] * 300, 4, 30, qual_table=table)
    assert r.voters.tolist() == [301] and r.qual.tolist() == [int(table[255])] * 4
    r = cs.round_host([b"ACGT"], [b"ACGT"] * 254, [0] * 254, 4, 30, qual_table=table, tmpl_counts=0)
    assert r.qual.tolist() == [int(table[254])] * 4


def test_qual_lies_like_cons_over_several_groups():
    tmpls = [b"ACGTACGTAC", b"ACGTCA", b"ACGACA", b"GGGG"]
    members = [b"ACGAACGTAC"] * 3 + [b"ACGCA"] * 3 + [b"ACGTACA"] * 3
    groups = [0] * 3 + [1] * 3 + [2] * 3
    r = cs.round_host(tmpls, members, groups, 4, 30, qual_table=MARGIN)
    assert r.lens.tolist() == [10, 5, 7, 4] and r.qual.size == r.cons.size == 26
    assert r.qual.tolist() == [4, 4, 4, 2, 4, 4, 4, 4, 4, 4] + [4] * 5 + [4, 4, 4, 2, 4, 4, 4] + [1] * 4
    # without a table: today's Round, qual None; the other fields are the same
    plain = cs.round_host(tmpls, members, groups, 4, 30)
    assert plain.qual is None and plain.cons.tobytes() == r.cons.tobytes() and np.array_equal(plain.voters, r.voters)
    assert cs.Round(1, 2, 3, 4, 5, 6).qual is None
    # no groups, no members: the library's no-op
    assert cs.round_host([], [], [], 4, 30, qual_table=MARGIN).qual.size == 0
    assert cs.round_host([b"ACGT"], [], [], 4, 30, qual_table=MARGIN).qual.size == 0


# ---- the rounds ---------------------------------------------------------------------------------------------------------------------
def _groups(lists):
    reads = [s for group in lists for s in group]
    off = np.concatenate([[0], np.cumsum([len(s) + 1 for s in reads])])[:-1].astype(np.int64)
    arena = np.frombuffer(b"".join(s + b"-" for s in reads), dtype=np.uint8)
    groups, at = [], 0
    for g, group in enumerate(lists):
        groups.append((g + 1, "K%d" % g, list(range(at, at + len(group)))))
        at += len(group)
    return groups, arena, off, np.array([len(s) for s in reads], dtype=np.int64)


GOOD, ERR = b"ACGTACGTACGTAAC", b"ACGTACCTACGTAAC"          # ERR: base 6 substituted


def test_the_qualities_travel_through_the_rounds():
    # group 1: three equal reads -- round 1 returns its template and ends the group with that round's qualities (3 : 0).
    # group 2: the template (the second read) holds an error the two others outvote 2 : 1; round 2 runs on the corrected
    # template as an earlier consensus with all three reads as members: 2 : 1 again in column 6, 3 : 0 elsewhere.
    # group 3: too few reads.
    out = cs.call_groups(*_groups([[GOOD] * 3, [GOOD, ERR, GOOD], [GOOD] * 2]), band=4, rounds=5, qual_table=MARGIN)
    assert [(r["rounds"], r["status"], r["sequence"]) for r in out] == [(1, "called", GOOD), (2, "called", GOOD), (0, "few_reads", None)]
    assert out[0]["quality"] == bytes([3] * 15)
    assert out[1]["quality"] == bytes([3] * 6 + [1] + [3] * 8)
    assert out[2]["quality"] is None
    # one round: the qualities of round 1, where the template is a read of the group
    one = cs.call_groups(*_groups([[GOOD, ERR, GOOD, GOOD]]), band=4, rounds=1, qual_table=MARGIN)
    assert one[0]["sequence"] == GOOD and one[0]["quality"] == bytes([4] * 6 + [2] + [4] * 8)
    # two rounds: round 2 replaces them with its own -- the same evidence, since round 1's template is a voter and round 2's
    # members are all four reads
    two = cs.call_groups(*_groups([[GOOD, ERR, GOOD, GOOD]]), band=4, rounds=2, qual_table=MARGIN)
    assert two[0]["rounds"] == 2 and two[0]["quality"] == bytes([4] * 6 + [2] + [4] * 8)
    # without a table: today's rows, no `quality`
    plain = cs.call_groups(*_groups([[GOOD] * 3, [GOOD, ERR, GOOD], [GOOD] * 2]), band=4, rounds=5)
    assert all("quality" not in r for r in plain)
    assert [{k: v for k, v in r.items() if k != "quality"} for r in out] == plain
    with pytest.raises(ValueError):
        cs.call_groups(*_groups([[GOOD] * 3]), band=4, qual_table=MARGIN[:100])


def test_a_strand_1_template_read_reverses_the_qualities():
    orig = b"ACGGTCATTGCAGGCTAAGC"
    err = orig[:5] + b"A" + orig[6:]                         # base 5: C -> A
    assert orig[5:6] == b"C" and len(orig) == 20
    # the lower median of three equal lengths is the second read: the template read is of strand 1, so round 1 runs in its
    # orientation, where the error lies at base 20 - 1 - 5 = 14, and its consensus and qualities are turned round afterwards
    lists = [[orig, cs.reverse_complement(err), orig]]
    want = bytes([3] * 5 + [1] + [3] * 14)
    for rounds in (1, 2):
        out = cs.call_groups(*_groups(lists), band=4, rounds=rounds, read_strand=[0, 1, 0], qual_table=MARGIN)
        assert out[0]["sequence"] == orig and out[0]["minus"] == 1 and out[0]["rounds"] == rounds
        assert out[0]["quality"] == want, (rounds, list(out[0]["quality"]))
    # the round itself, in the template read's orientation
    r = cs.round_host([cs.reverse_complement(err)], [orig, orig], [0, 0], 4, 30, member_strand=[1, 1], qual_table=MARGIN)
    assert r.cons.tobytes() == cs.reverse_complement(orig) and r.qual.tolist() == [3] * 14 + [1] + [3] * 5
    # a strand-0 template read among strand-1 members: nothing is turned
    out = cs.call_groups(*_groups([[cs.reverse_complement(orig), err, cs.reverse_complement(orig)]]), band=4, rounds=1,
                         read_strand=[1, 0, 1], qual_table=MARGIN)
    assert out[0]["sequence"] == orig and out[0]["quality"] == want and out[0]["minus"] == 2


# ---- writers ------------------------------------------------------------------------------------------------------------------------
ROWS = [dict(group=1, representative="AAAA+CC", members=5, used=4, rejected=1, skipped=0, rounds=2, length=6, status="called",
             sequence=b"ACGTCA", quality=bytes([0, 9, 10, 41, 60, 93])),
        dict(group=2, representative="GGGG+TT", members=2, used=0, rejected=0, skipped=0, rounds=0, length=0, status="few_reads",
             sequence=None, quality=None),
        dict(group=3, representative="CCCC+AA", members=3, used=3, rejected=0, skipped=0, rounds=1, length=2, status="called",
             sequence=b"GG", quality=bytes([20, 20]))]


def test_fastq_text_and_the_reports_two_columns():
    assert cs.fastq_text(ROWS) == ("@umi_group_1 key=AAAA+CC reads=5 used=4 rounds=2 length=6\nACGTCA\n+\n!*+J]~\n"
                                   "@umi_group_3 key=CCCC+AA reads=3 used=3 rounds=1 length=2\nGG\n+\n55\n")
    # 1 + 10^-0.9 + 0.1 + 10^-4.1 + 10^-6 + 10^-9.3 = 1.22597...; two bases below Q10
    assert cs.report_text(ROWS) == ("#group\trepresentative\tmembers\tused\trejected\tskipped\trounds\tlength\tstatus\texpected_errors\tlow_qual\n"
                                    "1\tAAAA+CC\t5\t4\t1\t0\t2\t6\tcalled\t1.226\t2\n"
                                    "2\tGGGG+TT\t2\t0\t0\t0\t0\t0\tfew_reads\t0.000\t0\n"
                                    "3\tCCCC+AA\t3\t3\t0\t0\t1\t2\tcalled\t0.020\t0\n")
    stranded = [dict(r, minus=k) for k, r in enumerate(ROWS)]
    text = cs.report_text(stranded)
    assert text.splitlines()[0].endswith("\tstatus\tminus\texpected_errors\tlow_qual")
    assert text.splitlines()[1].endswith("\tcalled\t0\t1.226\t2") and text.splitlines()[3].endswith("\tcalled\t2\t0.020\t0")
    assert cs.fastq_text(stranded).startswith("@umi_group_1 key=AAAA+CC reads=5 minus=0 used=4 rounds=2 length=6\n")
    # rows without qualities: today's report
    plain = [{k: v for k, v in r.items() if k != "quality"} for r in ROWS]
    assert cs.report_text(plain).splitlines()[0].endswith("\tstatus") and cs.report_text([]) == "#" + "\t".join(cs.REPORT_COLUMNS) + "\n"
    assert cs.report_text([], quality=True).rstrip("\n").endswith("low_qual")


# ---- the runner on the stand-in: the host route ---------------------------------------------------------------------------------------
def _run(tmp_path, tag, **kw):
    from porechop_amd import runner
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(ccase.build()))
    out = tmp_path / ("out_%s.fastq" % tag)
    opts = runner.Options()
    opts.check_reads = 3
    res = runner.run(str(inp), output=str(out), options=opts, aligner=ccase.ConsensusAligner(), adapter_panel=umi_runner_case.adapter_sets(),
                     wildcards=True, **kw)
    return res, out


def _phred33(values):
    return bytes(v + 33 for v in values).decode("ascii")


# tests/consensus_case.py's two molecules at the default table (1, 10, 25, 41, 56, 60).
# Molecule A ends in round 2: the original as an earlier consensus, members A1 A2 A3 A4 (X is rejected) -- 4 : 0 is Q56, and
# the columns of A3's and A4's substitutions (bases 60 and 100 of the body, 58 and 98 of the trimmed sequence) 3 : 1, Q25.
QUAL_A = [56] * 236
QUAL_A[58] = QUAL_A[98] = 25
# Molecule D ends in round 1: D1 is the template and a voter, 3 : 0 is Q41; D2 lacks base 150 of the body (148 of the sequence):
# two bases against one deletion there, Q10.  D3's inserted base is not emitted and costs no column a vote.
QUAL_D = [41] * 236
QUAL_D[148] = 10
FASTQ = ("@" + ccase.FASTA.splitlines()[0][1:] + "\n" + ccase.FASTA.splitlines()[1] + "\n+\n" + _phred33(QUAL_A) + "\n" +
         "@" + ccase.FASTA.splitlines()[2][1:] + "\n" + ccase.FASTA.splitlines()[3] + "\n+\n" + _phred33(QUAL_D) + "\n")
# 234 x 10^-5.6 + 2 x 10^-2.5 = 0.00691; 235 x 10^-4.1 + 10^-1 = 0.11867
TSV_Q = "".join(line + tail + "\n" for line, tail in zip(ccase.TSV.splitlines(), (
    "\texpected_errors\tlow_qual", "\t0.007\t0", "\t0.119\t0", "\t0.000\t0", "\t0.000\t0")))


def test_the_case_states_what_it_says():
    # the deletion of D2 cannot slide: the bases on either side of base 148 differ from it, so the column is the one stated
    seq = ccase.ORIG_D[2:-2]
    assert seq[147] != seq[148] != seq[149]


def test_runner_writes_the_stated_fastq(tmp_path):
    fa, fq, tsv = tmp_path / "cons.fasta", tmp_path / "cons.fastq", tmp_path / "cons.tsv"
    res, out = _run(tmp_path, "q", umi=True, umi_consensus=str(fa), umi_consensus_fastq=str(fq), umi_consensus_report=str(tsv))
    assert fq.read_text() == FASTQ
    assert fa.read_text() == ccase.FASTA and tsv.read_text() == TSV_Q
    assert [r["sequence"] for r in res.consensus] == ccase.SEQUENCES
    assert [r["quality"] for r in res.consensus] == [bytes(QUAL_A), bytes(QUAL_D), None, None]
    # the FASTQ alone makes the consensus run; the report needs only one of the two
    fq.unlink(), fa.unlink(), tsv.unlink()
    res2, out2 = _run(tmp_path, "alone", umi=True, umi_consensus_fastq=str(fq), umi_consensus_report=str(tsv))
    assert fq.read_text() == FASTQ and tsv.read_text() == TSV_Q and not fa.exists() and out2.read_bytes() == out.read_bytes()
    # another table: every vote wrong half the time, capped at 20 -- 1, 3, 7, 12, 18, 20
    res3, _ = _run(tmp_path, "half", umi=True, umi_consensus_fastq=str(fq), umi_consensus_vote_err_pct=50, umi_consensus_max_qual=20)
    assert sorted(set(res3.consensus[0]["quality"])) == [7, 18] and sorted(set(res3.consensus[1]["quality"])) == [3, 12]
    res4, _ = _run(tmp_path, "cap", umi=True, umi_consensus_fastq=str(fq), umi_consensus_max_qual=30)
    assert sorted(set(res4.consensus[0]["quality"])) == [25, 30]


def test_without_the_new_options_the_run_writes_todays_bytes(tmp_path):
    fa, tsv = tmp_path / "cons.fasta", tmp_path / "cons.tsv"
    res, out = _run(tmp_path, "plain", umi=True, umi_consensus=str(fa), umi_consensus_report=str(tsv))
    assert fa.read_text() == ccase.FASTA and tsv.read_text() == ccase.TSV
    assert all("quality" not in r for r in res.consensus)
    fq = tmp_path / "cons.fastq"
    _res, out_q = _run(tmp_path, "withq", umi=True, umi_consensus=str(fa), umi_consensus_fastq=str(fq))
    assert out_q.read_bytes() == out.read_bytes() and fa.read_text() == ccase.FASTA


def test_usage_errors(tmp_path):
    from porechop_amd import runner
    fq, fa = tmp_path / "c.fastq", tmp_path / "c.fasta"
    with pytest.raises(runner.UsageError, match="--umi_consensus_fastq needs --umi"):
        _run(tmp_path, "e1", umi_consensus_fastq=str(fq))
    with pytest.raises(runner.UsageError, match="--umi_consensus_report needs --umi_consensus"):
        _run(tmp_path, "e2", umi=True, umi_consensus_report=str(tmp_path / "c.tsv"))
    for kw, word in ((dict(umi_consensus_vote_err_pct=0), "vote_err_pct"), (dict(umi_consensus_vote_err_pct=51), "vote_err_pct"),
                     (dict(umi_consensus_vote_err_pct=2.5), "vote_err_pct"), (dict(umi_consensus_max_qual=0), "max_qual"),
                     (dict(umi_consensus_max_qual=94), "max_qual"), (dict(umi_consensus_band=128), "band")):
        with pytest.raises(runner.UsageError, match=word):
            _run(tmp_path, "e3", umi=True, umi_consensus_fastq=str(fq), **kw)
    # either of the two without the FASTQ
    for kw in (dict(umi_consensus_vote_err_pct=20), dict(umi_consensus_max_qual=40)):
        with pytest.raises(runner.UsageError, match="need --umi_consensus_fastq"):
            _run(tmp_path, "e4", umi=True, umi_consensus=str(fa), **kw)
        with pytest.raises(runner.UsageError, match="need --umi_consensus_fastq"):
            _run(tmp_path, "e5", umi=True, **kw)
    inp = tmp_path / "reads.fastq"
    with pytest.raises(runner.UsageError, match="streamed"):
        runner.run_streamed(str(inp), str(tmp_path / "out_s.fastq"), None, runner.Options(), aligner=ccase.ConsensusAligner(),
                            adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, umi=True, umi_consensus_fastq=str(fq))
    with pytest.raises(runner.UsageError, match="sharded"):
        runner._check_umi_consensus_options(True, None, None, True, (3, 256, 64, 2, 30, 65535), str(fq), 10, 60)
    assert not fq.exists() and not fa.exists() and not list(tmp_path.glob("out_*"))
    # a refusal after a file of the run has been written removes that file: more distinct keys than allowed
    rep = tmp_path / "umis.tsv"
    with pytest.raises(runner.UsageError, match="--umi_group_max_keys"):
        _run(tmp_path, "e6", umi=True, umi_report=str(rep), umi_consensus_fastq=str(fq), umi_group_max_keys=2)
    assert not fq.exists() and not list(tmp_path.glob("out_*"))


def test_a_failure_while_writing_leaves_no_file_behind(tmp_path):
    """The FASTA is written first; the FASTQ's path is a directory: the FASTA is removed again."""
    fa, fq = tmp_path / "c.fasta", tmp_path / "is_a_dir"
    fq.mkdir()
    with pytest.raises(OSError):
        _run(tmp_path, "e7", umi=True, umi_consensus=str(fa), umi_consensus_fastq=str(fq))
    assert not fa.exists()


def test_a_large_input_is_not_streamed_with_the_fastq(tmp_path, monkeypatch):
    fq = tmp_path / "c.fastq"
    monkeypatch.setenv("PC_STREAM_BLOCK_BYTES", "1500")
    _run(tmp_path, "big", umi=True, umi_consensus_fastq=str(fq))
    assert fq.read_text() == FASTQ


def test_command_line_options(tmp_path):
    from porechop_amd import custom
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq", "--wildcards", "--umi", "--umi_consensus_fastq", "c.fq",
                                                 "--umi_consensus_vote_err_pct", "5", "--umi_consensus_max_qual", "40"])
    assert (a.umi_consensus_fastq, a.umi_consensus_vote_err_pct, a.umi_consensus_max_qual) == ("c.fq", 5, 40)
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq"])
    assert (a.umi_consensus_fastq, a.umi_consensus_vote_err_pct, a.umi_consensus_max_qual) == (None, None, None)
    kit = tmp_path / "umi.fasta"
    kit.write_text(">UMI kit_start\n%s\n>UMI kit_end\n%s\n" % (umi_runner_case.START, umi_runner_case.END))
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(ccase.build()))
    common = ["-i", str(inp), "-o", str(tmp_path / "o.fastq"), "--adapters", str(kit), "--only_custom", "--wildcards"]
    fq = tmp_path / "c.fq"
    for extra in (["--umi_consensus_fastq", str(fq)],                                              # --umi is missing
                  ["--umi", "--umi_consensus", str(tmp_path / "c.fa"), "--umi_consensus_max_qual", "60"],      # given without the FASTQ
                  ["--umi", "--umi_consensus_vote_err_pct", "10"],
                  ["--umi", "--umi_consensus_fastq", str(fq), "--umi_consensus_vote_err_pct", "60"]):
        with pytest.raises(SystemExit) as e:
            custom.main(common + extra)
        assert e.value.code not in (0, None), extra
    assert not fq.exists() and "--umi_consensus_fastq" in custom.__doc__


# ---- the property that keeps the rule honest -----------------------------------------------------------------------------------------
def substituted_copies(seed, copies=3, length=300, rate=0.10):
    rng = random.Random(seed)
    original = "".join(rng.choice("ACGT") for _ in range(length))
    reads = ["".join(rng.choice([b for b in "ACGT" if b != ch]) if rng.random() < rate else ch for ch in original).encode()
             for _ in range(copies)]
    return original.encode(), reads


PROPERTY_SEEDS = range(20)


def test_wrong_bases_carry_lower_qualities_than_right_ones():
    """20 seeded groups of 3 copies of a 300-base original with 10 % SUBSTITUTIONS only, two rounds, the default table.  Over the
    groups whose consensus has 300 bases, the mean quality of the positions that differ from the original is strictly below
    that of the positions that agree, and at least 50 differing positions exist.
    Counted on the model as it stands (seeds 0 .. 19; the template's vote is no evidence in round 2): 20 of 20 groups at 300
    bases, 171 differing positions of mean quality 5.6 against 33.2 at the 5 829 agreeing ones (printed below)."""
    table = cs.quality_table()
    wrong, right, kept = [], [], 0
    for seed in PROPERTY_SEEDS:
        original, reads = substituted_copies(seed)
        row = cs.call_groups(*_groups([reads]), rounds=2, qual_table=table)[0]
        assert row["status"] == "called" and len(row["quality"]) == row["length"]
        if row["length"] != 300:
            continue
        kept += 1
        differs = np.frombuffer(row["sequence"], dtype=np.uint8) != np.frombuffer(original, dtype=np.uint8)
        q = np.frombuffer(row["quality"], dtype=np.uint8)
        wrong += q[differs].tolist()
        right += q[~differs].tolist()
    print("groups at 300 bases: %d of %d; wrong positions %d, mean quality %.1f; right positions %d, mean quality %.1f" % (
        kept, len(PROPERTY_SEEDS), len(wrong), np.mean(wrong), len(right), np.mean(right)))
    assert len(wrong) >= 50
    assert np.mean(wrong) < np.mean(right)
