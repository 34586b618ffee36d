"""The Python side of the middle hits' paths, without a GPU: the report's header and rows with the middle_cigars column
(hand-made RunExplain), the interval / mask tables Pipeline.middle_hit_paths hands to Aligner.middle_paths (hand-made hit
list whose reads interleave across rounds), and the option's usage error."""
import numpy as np
import pytest
import torch

from porechop_amd import runner
from porechop_amd.pipeline import middle_mask_tables

BASE = "#" + "\t".join(runner.REPORT_COLUMNS)


def test_the_four_headers():
    assert runner.report_header() == BASE + "\n" and len(runner.REPORT_COLUMNS) == 17
    assert runner.report_header(True) == runner.report_header(paths=True) == BASE + "\tstart_cigars\tend_cigars\n"
    assert runner.report_header(False, True) == runner.report_header(middle_paths=True) == BASE + "\tmiddle_cigars\n"
    assert runner.report_header(True, True) == BASE + "\tstart_cigars\tend_cigars\tmiddle_cigars\n"


def explain(hit_cigars=None, middle_cigars=None):
    """Three reads: the first with two middle hits, the second with none, the third with one; one end alignment (read 0)."""
    summary = np.zeros((3, 12), dtype=np.int32)
    summary[:, 4:10] = -1
    summary[0, 0] = 31
    hits = np.array([[0, 2, 30, 26, 28, 28]], dtype=np.int32)
    middle = np.array([[1, 500, 522, ], [0, 530, 558], [0, 90, 118]], dtype=np.int64)
    return runner.RunExplain(summary, np.zeros((3, 4)), np.array([0, 1, 1, 1], dtype=np.int64), hits, [0], ["SetA"], None,
                             np.array([0, 2, 2, 3], dtype=np.int64), middle, np.array([95.454545, 100.0, 89.285714]), ["Top", "Bottom"],
                             hit_cigars=hit_cigars, middle_cigars=middle_cigars)


def test_rows_with_and_without_the_column():
    names, lengths = ["r0", "r1", "r2"], [1000, 800, 400]
    plain = runner.report_rows(explain(), names, lengths).split("\n")
    ends = runner.report_rows(explain(hit_cigars=["2|0|28="]), names, lengths).split("\n")
    mid_cigars = ["500|0|10=1X11=", "530|0|28=", "90|0|12=1I16="]
    mids = runner.report_rows(explain(middle_cigars=mid_cigars), names, lengths).split("\n")
    both = runner.report_rows(explain(hit_cigars=["2|0|28="], middle_cigars=mid_cigars), names, lengths).split("\n")
    assert plain[-1] == ends[-1] == mids[-1] == both[-1] == "" and len(plain) == 4
    assert all(len(r.split("\t")) == 17 for r in plain[:-1])
    assert plain[0].split("\t")[6] == "Bottom|500|522|95.454545;Top|530|558|100.000000"
    # one more column, entry for entry with middle_hits in the read's discovery order, '.' for a read without hits
    want = ["500|0|10=1X11=;530|0|28=", ".", "90|0|12=1I16="]
    for r in range(3):
        assert mids[r] == plain[r] + "\t" + want[r]
        assert ends[r].split("\t")[:17] == plain[r].split("\t") and len(ends[r].split("\t")) == 19
        assert both[r] == ends[r] + "\t" + want[r]                  # behind start_cigars / end_cigars


def test_concatenated_blocks_chain_the_column():
    a, b = explain(middle_cigars=["a0", "a1", "a2"]), explain(middle_cigars=["b0", "b1", "b2"])
    ex = runner._concat_explain([a, b])
    assert ex.middle_cigars == ["a0", "a1", "a2", "b0", "b1", "b2"] and ex.middle_first.tolist() == [0, 2, 2, 3, 5, 5, 6]
    rows = runner.report_rows(ex, ["r%d" % i for i in range(6)], [1000] * 6).split("\n")
    assert [r.split("\t")[17] for r in rows[:-1]] == ["a0;a1", ".", "a2", "b0;b1", ".", "b2"]
    assert runner._concat_explain([explain(), explain()]).middle_cigars is None


def test_mask_tables_of_reads_that_interleave_across_rounds():
    """Phase C lists hits round by round: round 0 of reads 7, 2, 9, round 1 of reads 2 and 7, round 2 of read 7.  The table
    holds every interval once, grouped by read in discovery order; a hit of rank k sees the k rows before its own."""
    read = torch.tensor([7, 2, 9, 2, 7, 7], dtype=torch.int64)
    start = torch.tensor([100, 40, 5, 300, 700, 10], dtype=torch.int32)
    end = torch.tensor([128, 62, 33, 322, 728, 38], dtype=torch.int32)
    intervals, base, count = middle_mask_tables(read, start, end)
    assert intervals.dtype == torch.int32 and base.dtype == torch.int64 and count.dtype == torch.int32
    assert intervals.tolist() == [[40, 62], [300, 322], [100, 128], [700, 728], [10, 38], [5, 33]]
    assert base.tolist() == [2, 0, 5, 0, 2, 2] and count.tolist() == [0, 0, 0, 1, 1, 2]
    # the rows a hit sees are exactly its read's earlier hits, in order
    for h in range(6):
        earlier = [k for k in range(h) if int(read[k]) == int(read[h])]
        rows = intervals[int(base[h]):int(base[h]) + int(count[h])].tolist()
        assert rows == [[int(start[k]), int(end[k])] for k in earlier]
    e_i, e_b, e_c = middle_mask_tables(read[:0], start[:0], end[:0])
    assert tuple(e_i.shape) == (0, 2) and e_b.numel() == 0 and e_c.numel() == 0
    one = middle_mask_tables(read[:1], start[:1], end[:1])
    assert one[0].tolist() == [[100, 128]] and one[1].tolist() == [0] and one[2].tolist() == [0]


def test_middle_paths_need_a_report(tmp_path):
    with pytest.raises(runner.UsageError):
        runner.run(str(tmp_path / "none.fastq"), output=str(tmp_path / "out.fastq"), report_middle_paths=True)
    with pytest.raises(runner.UsageError):
        runner.run(str(tmp_path / "none.fastq"), output=str(tmp_path / "out.fastq"), report_paths=True, report_middle_paths=True)
