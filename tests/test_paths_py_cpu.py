"""The host-side pieces around alignment paths, without a GPU: decode_paths / cigar / render_alignment on hand-written
heads and dwords, the Python path checker against the host build of pc_paths.h, and report_rows with and without the
per-hit path list."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from porechop_amd import runner
from porechop_amd.batch import cigar, decode_paths, expand_cigar, render_alignment
from tests import pathcheck

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words_of(forward, pitch=None):
    """The dwords the kernel writes for a forward operation string: traceback order, sixteen to a word, lowest bits first."""
    codes = ["=XID".index(c) for c in reversed(forward)]
    w = [0] * max(1, (len(codes) + 15) // 16 if pitch is None else pitch)
    for k, c in enumerate(codes):
        w[k // 16] |= c << (2 * (k % 16))
    return w


def pattern(n):
    return "".join("=XID"[(k * 7 + k // 3) % 4] for k in range(n))


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33])
def test_decode_and_cigar_on_hand_written_words(n):
    fwd = pattern(n)
    w = words_of(fwd, pitch=3)
    head = [n, 2, 0, 1]
    for dtype in (np.uint32, np.int32):                      # torch hands the words out as int32
        ops = np.array([w], dtype=np.uint32).view(dtype) if dtype is np.int32 else np.array([w], dtype=np.uint32)
        assert decode_paths([head], ops) == [fwd]
    assert expand_cigar(cigar(fwd)) == fwd
    if n == 0:
        assert cigar(fwd) == ""
    # the first operation of the traceback is the path's LAST step and sits in the lowest bits of word 0
    if n:
        assert "=XID"[w[0] & 3] == fwd[-1]
    if n > 16:
        assert "=XID"[w[1] & 3] == fwd[-17]


def test_words_with_the_top_bit_set_and_several_rows():
    a, b = "=" + "D" * 16, "I" * 7
    ops = np.array([words_of(a, 2), words_of(b, 2)], dtype=np.uint32)
    assert ops[0, 0] == 0xFFFFFFFF
    assert decode_paths([[17, 0, 0, 1], [7, 0, 3, 1]], ops.view(np.int32)) == [a, b]
    assert decode_paths(np.zeros((0, 4), dtype=np.int32), np.zeros((0, 5), dtype=np.int32)) == []
    with pytest.raises(ValueError):
        decode_paths([[33, 0, 0, 0]], ops[:1])


def test_cigar_strings():
    assert cigar("=================X====II======") == "17=1X4=2I6="
    assert cigar("DDDD") == "4D" and cigar("IDID") == "1I1D1I1D"
    assert expand_cigar("17=1X4=2I6=") == "=================X====II======"
    for bad in ("3", "=", "3Q", "3=4"):
        with pytest.raises(ValueError):
            expand_cigar(bad)
    with pytest.raises(ValueError):
        cigar("==M")


def test_render_alignment():
    # the read from its base 2 (ACGTTACG...) against the adapter from its base 2 (ACGTACCG...)
    text = render_alignment("TTACGTTACGA", b"GGACGTACCGA", (9, 2, 2, 2), "==IX===D=")
    assert text.split("\n") == ["ACGTTAC-G",
                                "||  ||| |",
                                "AC-GTACCG"]
    # gaps only, and an empty path
    assert render_alignment("ACGT", "TT", (3, 1, 0, 2), "IDI").split("\n") == ["C-G", "   ", "-T-"]
    assert render_alignment("ACGT", "TT", (0, 0, 2, 0), "") == "\n\n"
    with pytest.raises(ValueError):
        render_alignment("ACGT", "TT", (1, 0, 0, 0), "M")


def test_python_checker_against_the_host_build(oracle):
    """tests/pathcheck.py -- what the GPU tests hold every returned path to -- on 300 cases dumped by the host build of
    pc_paths.h (tests/host/test_paths.cpp, dump mode), and on damaged copies of them, which it must refuse."""
    with tempfile.TemporaryDirectory() as tmp:
        exe, obj = os.path.join(tmp, "test_paths"), os.path.join(tmp, "pc_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-c", os.path.join(REPO, "oracle", "pc_oracle.c"), "-o", obj])
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "porechop_amd", "csrc"), "-I", os.path.join(REPO, "oracle"),
                               os.path.join(REPO, "tests", "host", "test_paths.cpp"), obj, "-o", exe])
        out = subprocess.run([exe, "300", "7", "dump"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bad=0 " in out.stdout
    seen = refused = 0
    for line in out.stdout.splitlines():
        if not line.startswith("CASE "):
            continue
        f = line.split()
        rd, ad = ("" if x == "." else x for x in f[1:3])
        sc = tuple(int(x) for x in f[3:7])
        rec, head = [int(x) for x in f[7:15]], [int(x) for x in f[15:19]]
        fwd = "" if f[19] == "." else f[19]
        want = oracle.align_raw(rd, ad, sc)
        assert pathcheck.oracle_record(want) == rec
        pathcheck.check_path(rd, ad, sc, rec, head, fwd, want)
        seen += 1
        if len(fwd) >= 2 and "=" in fwd:
            k = fwd.index("=")
            for damaged in (fwd[:k] + "X" + fwd[k + 1:], fwd[1:], fwd + "I"):
                h = [len(damaged)] + head[1:]
                with pytest.raises(AssertionError):
                    pathcheck.check_path(rd, ad, sc, rec, h, damaged, want)
                refused += 1
    assert seen == 300 and refused > 100


def hand_made_explain(cigars):
    # three reads: two start hits and one end hit; nothing; one end hit
    hits = np.array([[0, 3, 31, 27, 28, 28], [2, 0, 24, 22, 24, 24], [1, 100, 128, 26, 28, 28], [1, 90, 150, 50, 60, 28]], dtype=np.int32)
    summary = np.zeros((3, 12), dtype=np.int32)
    summary[:, 4:10] = -1
    summary[0, :4] = (33, 52, 2, 1)
    summary[2, :4] = (0, 62, 0, 1)
    return runner.RunExplain(summary, np.zeros((3, 4)), np.array([0, 3, 3, 4], dtype=np.int64), hits, [0, 1, 0], ["SQK-NSK007", "SQK-NSK007", "Rapid"],
                             None, np.zeros(4, dtype=np.int64), np.zeros((0, 3), dtype=np.int64), np.zeros(0), [], None, None, cigars)


def test_report_rows_with_and_without_the_per_hit_list():
    names, lengths = ["r0 x", "r1", "r2"], [1000, 20, 500]
    plain = runner.report_rows(hand_made_explain(None), names, lengths)
    # today's bytes: 17 columns, nothing appended
    assert plain == (
        "r0 x\t1000\t33\t52\tSQK-NSK007|96.428571|96.428571|3|31;Rapid|91.666667|91.666667|0|24\tSQK-NSK007|92.857143|92.857143|100|128\t."
        + "\t." * 10 + "\n"
        "r1\t20\t0\t0\t.\t.\t." + "\t." * 10 + "\n"
        "r2\t500\t0\t62\t.\tSQK-NSK007|178.571429|83.333333|90|150\t." + "\t." * 10 + "\n")
    assert runner.report_header() == "#" + "\t".join(runner.REPORT_COLUMNS) + "\n" and len(runner.REPORT_COLUMNS) == 17
    cig = ["3|0|17=1X10=", "0|2|22=1I1=1D", "100|0|26=2X", "90|0|50=10X"]
    with_paths = runner.report_rows(hand_made_explain(cig), names, lengths)
    assert runner.report_header(True) == "#" + "\t".join(runner.REPORT_COLUMNS + ["start_cigars", "end_cigars"]) + "\n"
    rows_a, rows_b = plain.splitlines(), with_paths.splitlines()
    assert len(rows_a) == len(rows_b) == 3
    for a, b in zip(rows_a, rows_b):
        cols = b.split("\t")
        assert len(cols) == 19 and "\t".join(cols[:17]) == a
        # aligned entry for entry
        for al_col, cg_col in ((cols[4], cols[17]), (cols[5], cols[18])):
            assert (al_col == ".") == (cg_col == ".")
            if al_col != ".":
                assert len(al_col.split(";")) == len(cg_col.split(";"))
    assert rows_b[0].split("\t")[17:] == ["3|0|17=1X10=;0|2|22=1I1=1D", "100|0|26=2X"]
    assert rows_b[1].split("\t")[17:] == [".", "."]
    assert rows_b[2].split("\t")[17:] == [".", "90|0|50=10X"]
