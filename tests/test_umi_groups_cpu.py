"""UMI groups without a GPU (porechop_amd/umi_groups.py and the runner's route to it): the keys of the reads, the keys that
cannot be linked, the numpy neighbours against discover.edit_distance, the two grouping rules on cases stated by hand, the
runner on the stand-in of tests/umi_groups_aligner.py -- which has no umi_neighbours, so the host route is taken -- with the
groups TSV stated by hand, every refusal and the command line's options."""
import os
import random

import numpy as np
import pytest

from porechop_amd import umi_groups as ug
from tests import umi_groups_aligner as gcase
from tests import umi_runner_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _umi(bases):
    return None if bases is None else ("kit", 0, len(bases), len(bases), bases)


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def test_read_keys_of_the_three_modes():
    umis = [(_umi("ACGT"), _umi("GGTT")), (_umi("acgu"), None), (None, _umi("ggUu")), (None, None), (_umi("AC"), _umi("NG"))]
    assert ug.read_keys(umis, "start") == ["ACGT", "ACGT", None, None, "AC"]
    assert ug.read_keys(umis, "end") == ["GGTT", None, "GGTT", None, "NG"]
    assert ug.read_keys(umis, "both") == ["ACGT+GGTT", None, None, None, "AC+NG"]
    with pytest.raises(ValueError):
        ug.read_keys(umis, "either")
    keys, counts, node = ug.unique_keys(ug.read_keys(umis, "start"))
    assert keys == ["ACGT", "AC"] and counts == [2, 1] and node == [0, 0, -1, -1, 1]


def test_keys_that_cannot_be_linked():
    assert ug.linkable("ACGT") and ug.linkable("AC+GT") and ug.linkable("A" * 64) and ug.linkable("A" * 32 + "+" + "C" * 32)
    assert not ug.linkable("") and not ug.linkable("+") and not ug.linkable("A" * 65) and not ug.linkable("A" * 33 + "+" + "C" * 32)
    assert not ug.linkable("ACNT") and not ug.linkable("AC+NT")
    # in a run they are nodes without edges: the N key is one edit from two others and joins neither
    umis = [(_umi("ACGT"), None)] * 3 + [(_umi("ACNT"), None), (_umi("A" * 65), None), (_umi("ACGA"), None)]
    per_read, rows = ug.assign(umis, ["r%d" % k for k in range(6)], "start", max_dist=2)
    assert per_read == [(1, "ACGT")] * 3 + [(3, "ACNT"), (2, "A" * 65), (1, "ACGT")]
    assert rows.splitlines()[3] == "r3\t3\tACNT\t1\t1\t1\tACNT"
    with pytest.raises(ValueError):
        ug.pack(["ACNT"])
    with pytest.raises(ValueError):
        ug.pack(["A" * 65])


def test_pack_layout():
    planes, lens = ug.pack(["", "A", "C", "G", "T", "ACGT", "AC+GT", "T" * 64])
    assert planes.dtype == np.uint64 and lens.dtype == np.int32 and lens.tolist() == [0, 1, 1, 1, 1, 4, 4, 64]
    assert planes.tolist() == [[0, 0], [0, 0], [1, 0], [0, 1], [1, 1], [0b1010, 0b1100], [0b1010, 0b1100], [2**64 - 1, 2**64 - 1]]
    planes, lens = ug.pack([])
    assert planes.shape == (0, 2) and lens.shape == (0,)
    # the base counts, and the order the keys go to the kernel in: by length, then by the counts of A, C, G
    keys = ["TTTT", "AACGT", "", "ACGT", "AAAA", "T" * 64, "CCAA"]
    planes, lens = ug.pack(keys)
    planes[1] |= np.uint64(0xFF) << np.uint64(40)                                # garbage above the length is not counted
    assert ug.composition(planes, lens).tolist() == [[0, 0, 0, 4], [2, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1], [4, 0, 0, 0], [0, 0, 0, 64], [2, 2, 0, 0]]
    assert [keys[k] for k in ug.kernel_order(planes, lens)] == ["", "TTTT", "ACGT", "CCAA", "AAAA", "AACGT", "T" * 64]


# ---- neighbours_host against the plain DP -----------------------------------------------------------------------------------------
def _seeded_keys(seed, n):
    rng = random.Random(seed)
    keys = []
    while len(keys) < n:
        if keys and rng.random() < 0.5:                              # a copy of an earlier key with 0..3 edits
            k = list(rng.choice(keys))
            for _ in range(rng.randrange(4)):
                kind, at = rng.randrange(3), rng.randrange(len(k) + 1)
                if kind == 0 and k:
                    k[min(at, len(k) - 1)] = rng.choice("ACGT")
                elif kind == 1 and len(k) < 64:
                    k.insert(at, rng.choice("ACGT"))
                elif k:
                    del k[min(at, len(k) - 1)]
            keys.append("".join(k))
        else:
            keys.append("".join(rng.choice("ACGT") for _ in range(rng.choice([0, 1, 5, 8, 12, 12, 12, 33, 64]))))
    return keys


@pytest.mark.parametrize("max_dist", [0, 2, 7])
def test_neighbours_host_against_the_plain_dp(max_dist):
    from porechop_amd.discover import edit_distance
    keys = _seeded_keys(17, 220)
    planes, lens = ug.pack(keys)
    want = [(i, j, d) for i in range(len(keys)) for j in range(i + 1, len(keys))
            for d in [edit_distance(keys[i], keys[j])] if d <= max_dist]
    assert len(want) > 50
    got = ug.neighbours_host(planes, lens, max_dist)
    assert got.dtype == np.int32 and got.tolist() == [list(w) for w in want]
    # garbage above the lengths changes nothing; a length outside 0..64 has no pairs
    rng = np.random.default_rng(3)
    dirty = planes | (rng.integers(0, 2**63, size=planes.shape, dtype=np.uint64) << np.uint64(1) & ~ug._len_mask(lens)[:, None])
    assert np.array_equal(ug.neighbours_host(dirty, lens, max_dist), got)
    bad = lens.copy()
    bad[5], bad[9] = 65, -1
    assert ug.neighbours_host(planes, bad, max_dist).tolist() == [list(w) for w in want if w[0] not in (5, 9) and w[1] not in (5, 9)]
    assert ug.neighbours_host(planes[:1], lens[:1], max_dist).shape == (0, 3) and ug.neighbours_host(planes[:0], lens[:0], 2).shape == (0, 3)


# ---- the two rules, on cases stated by hand ----------------------------------------------------------------------------------------
def test_equal_counts_are_two_groups_directional_and_one_cluster():
    keys, counts, pairs = ["ACGT", "ACGA"], [5, 5], [(0, 1, 1)]
    assert ug.group(keys, counts, pairs, "directional") == ([2, 1], ["ACGT", "ACGA"])          # 5 < 2 * 5 - 1; ACGA < ACGT founds first
    assert ug.group(keys, counts, pairs, "cluster") == ([1, 1], ["ACGA", "ACGA"])
    assert ug.group(keys, counts, pairs) == ug.group(keys, counts, pairs, "directional")
    with pytest.raises(ValueError):
        ug.group(keys, counts, pairs, "adjacency")


def test_a_chain_whose_middle_node_cannot_pass_the_count_on():
    # a (10) - b (1) - c (2): a takes b (10 >= 1), b does not take c (1 < 3), and c does not reach back into a's group
    keys, counts, pairs = ["AAAA", "AAAC", "AACC"], [10, 1, 2], np.array([[0, 1, 1], [1, 2, 1]])
    assert ug.group(keys, counts, pairs, "directional") == ([1, 1, 2], ["AAAA", "AAAA", "AACC"])
    assert ug.group(keys, counts, pairs, "cluster") == ([1, 1, 1], ["AAAA"] * 3)
    # a middle node of 2 reads before an end node of 1 passes the count on: 10 >= 2 * 2 - 1 and 2 >= 2 * 1 - 1
    assert ug.group(keys, [10, 2, 1], pairs, "directional") == ([1, 1, 1], ["AAAA"] * 3)


def test_a_tie_in_count_is_decided_by_key_order():
    keys, counts = ["CCCC", "AAAA", "GGGG"], [3, 3, 3]
    assert ug.group(keys, counts, np.zeros((0, 3), dtype=np.int32)) == ([2, 1, 3], ["CCCC", "AAAA", "GGGG"])
    # the founder of a component is its first node in that order
    assert ug.group(keys, counts, [(0, 2, 1)], "cluster") == ([2, 1, 2], ["CCCC", "AAAA", "CCCC"])


def test_a_node_two_founders_reach_goes_to_the_earlier_one():
    keys, counts, pairs = ["TTTT", "AAAA", "ATTT"], [10, 10, 1], [(0, 2, 1), (1, 2, 3)]
    assert ug.group(keys, counts, pairs, "directional") == ([2, 1, 1], ["TTTT", "AAAA", "AAAA"])
    keys, counts = ["AAAA", "TTTT", "ATTT"], [9, 10, 1]                                           # the larger count is earlier
    assert ug.group(keys, counts, [(0, 2, 3), (1, 2, 1)], "directional") == ([2, 1, 1], ["AAAA", "TTTT", "TTTT"])


# ---- the runner on the stand-in ------------------------------------------------------------------------------------------------------
def _run(tmp_path, tag, streamed=None, panel=None, **kw):
    from porechop_amd import runner
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(gcase.build()))
    out = tmp_path / ("out_%s.fastq" % tag)
    opts = runner.Options()
    opts.check_reads = 3
    common = dict(aligner=gcase.UmiGroupsAligner(), adapter_panel=panel or umi_runner_case.adapter_sets(), wildcards=True, **kw)
    if streamed:
        res = runner.run_streamed(str(inp), str(out), None, opts, block_bytes=streamed, **common)
        assert res is not None, "not streamed"
    else:
        res = runner.run(str(inp), output=str(out), options=opts, **common)
    return res, out


def test_runner_writes_the_stated_groups(tmp_path):
    tsv = tmp_path / "groups.tsv"
    res, out = _run(tmp_path, "groups", umi=True, umi_groups=str(tsv))
    assert tsv.read_text() == gcase.groups_text(gcase.ROWS_BOTH)
    assert res.umi_groups == gcase.GROUPS_BOTH
    assert "umi_groups" in res.seconds
    # the files are those of a run without the option; no header carries a group
    res_off, out_off = _run(tmp_path, "off", umi=True)
    assert out.read_bytes() == out_off.read_bytes() and res_off.umi_groups is None and "umi_groups" not in res_off.seconds
    assert res.umis == res_off.umis
    # the start UMIs alone; cluster gives the same groups here
    for method in ("directional", "cluster"):
        res, _ = _run(tmp_path, "start", umi=True, umi_groups=str(tsv), umi_group_by="start", umi_group_method=method)
        assert tsv.read_text() == gcase.groups_text(gcase.ROWS_START)
    # max_dist 0: K_A1 is no neighbour of K_A any more and founds a group of its own, before K_N (K_A1 > K_N as text: K_N is earlier)
    res, _ = _run(tmp_path, "exact", umi=True, umi_groups=str(tsv), umi_max_dist=0)
    assert res.umi_groups[3] == (4, gcase.K_A1) and res.umi_groups[7] == (3, gcase.K_N) and res.umi_groups[0] == (1, gcase.K_A)


@pytest.mark.parametrize("block", [1500, 4000])
def test_streamed_run_writes_the_same_bytes(tmp_path, block):
    tsv, tsv_s = tmp_path / "groups.tsv", tmp_path / "groups_streamed.tsv"
    whole, out = _run(tmp_path, "whole", umi=True, umi_groups=str(tsv))
    streamed, out_s = _run(tmp_path, "streamed", streamed=block, umi=True, umi_groups=str(tsv_s))
    assert tsv_s.read_bytes() == tsv.read_bytes() == gcase.groups_text(gcase.ROWS_BOTH).encode()
    assert out_s.read_bytes() == out.read_bytes()
    assert streamed.umi_groups == whole.umi_groups == gcase.GROUPS_BOTH


# ---- refusals and the command line ---------------------------------------------------------------------------------------------------
def test_usage_errors(tmp_path):
    from porechop_amd import runner
    from porechop_amd.pipeline import AdapterSet
    tsv = tmp_path / "g.tsv"
    with pytest.raises(runner.UsageError, match="--umi_groups needs --umi"):
        _run(tmp_path, "e1", umi_groups=str(tsv))
    with pytest.raises(runner.UsageError, match="--umi_group_by"):
        _run(tmp_path, "e2", umi=True, umi_groups=str(tsv), umi_group_by="either")
    with pytest.raises(runner.UsageError, match="--umi_group_method"):
        _run(tmp_path, "e3", umi=True, umi_groups=str(tsv), umi_group_method="adjacency")
    with pytest.raises(runner.UsageError, match="--umi_max_dist"):
        _run(tmp_path, "e4", umi=True, umi_groups=str(tsv), umi_max_dist=65)
    # a panel whose end adapter has no degenerate letter: "end" and "both" name a side without a span, None means "start"
    start_only = [AdapterSet(umi_runner_case.KIT, ("UMI_start", umi_runner_case.START), ("plain_end", "GCTAGTCAGGTCCTGATCCATGAGTC"))]
    for by in ("end", "both"):
        for streamed in (None, 1500):
            with pytest.raises(runner.UsageError, match="--umi_group_by %s needs degenerate letters in a end adapter" % by):
                _run(tmp_path, "e5", streamed=streamed, panel=start_only, umi=True, umi_groups=str(tsv), umi_group_by=by)
    assert not tsv.exists() and not list(tmp_path.glob("out_*"))
    res, _ = _run(tmp_path, "start_only", panel=start_only, umi=True, umi_groups=str(tsv))
    assert tsv.read_text() == gcase.groups_text(gcase.ROWS_START)
    tsv.unlink()
    # more distinct keys than allowed: the message names the option, and nothing is left behind
    for streamed in (None, 1500):
        for p in tmp_path.glob("out_*"):
            p.unlink()
        with pytest.raises(runner.UsageError, match="--umi_group_max_keys"):
            _run(tmp_path, "e6", streamed=streamed, umi=True, umi_groups=str(tsv), umi_group_max_keys=2)
        assert not tsv.exists() and not list(tmp_path.glob("out_*"))
    # the key that cannot be linked does not count: three linkable keys pass a limit of three
    _run(tmp_path, "limit", umi=True, umi_groups=str(tsv), umi_group_max_keys=3)
    assert tsv.read_text() == gcase.groups_text(gcase.ROWS_BOTH)
    assert "umi_groups" not in runner.Options.__dataclass_fields__


def test_command_line_options(tmp_path):
    from porechop_amd import custom
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq", "--wildcards", "--umi", "--umi_groups", "g.tsv", "--umi_group_by", "start",
                                                 "--umi_max_dist", "3", "--umi_group_method", "cluster", "--umi_group_max_keys", "1000"])
    assert (a.umi_groups, a.umi_group_by, a.umi_max_dist, a.umi_group_method, a.umi_group_max_keys) == ("g.tsv", "start", 3, "cluster", 1000)
    a = custom.build_custom_parser().parse_args(["-i", "x.fastq"])
    assert (a.umi_groups, a.umi_group_by, a.umi_max_dist, a.umi_group_method, a.umi_group_max_keys) == (None, None, 2, "directional", 1 << 20)
    for argv in (["--umi_group_by", "either"], ["--umi_group_method", "adjacency"]):
        with pytest.raises(SystemExit):
            custom.build_custom_parser().parse_args(["-i", "x.fastq"] + argv)
    fa = tmp_path / "umi.fasta"
    fa.write_text(">UMI kit_start\n%s\n>UMI kit_end\n%s\n" % (umi_runner_case.START, umi_runner_case.END))
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(gcase.build()))
    with pytest.raises(SystemExit) as e:
        custom.main(["-i", str(inp), "-o", str(tmp_path / "o.fastq"), "--adapters", str(fa), "--only_custom", "--wildcards",
                     "--umi_groups", str(tmp_path / "g.tsv")])
    assert "--umi_groups needs --umi" in str(e.value)
