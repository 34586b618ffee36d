"""Adapter discovery without a GPU: assemble() over the model's counts (tests/kmer_model.py) recovers planted adapters
character for character; its tie, ratio and length rules; the FASTA of adapter sets; Discovery.adapter_sets()."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kmer_model as km

from porechop_amd import discover as dv
from porechop_amd.discover import Discovery, Found, assemble


# ---- planted recovery ---------------------------------------------------------------------------------------------------
CASES = [(3000, 0.8, 0.08), (3000, 0.5, 0.12), (2000, 1.0, 0.0)]
_windows = {}


def windows_of(case, seed):
    """the reads of a case are made once and shared by the three k"""
    key = (case, seed)
    if key not in _windows:
        _windows[key] = km.end_windows(km.planted_reads(*case, seed))
    return _windows[key]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("k", [8, 10, 12])
@pytest.mark.parametrize("case", CASES)
def test_planted_adapters_are_recovered_exactly(case, k, seed):
    for windows, planted in zip(windows_of(case, seed), (km.Y_TOP, km.Y_BOTTOM)):
        codes, counts = km.count_sparse(windows, k)
        found = assemble(codes, counts, k, len(windows))
        assert [f.sequence for f in found] == [planted]
        assert found[0].peak >= found[0].support >= 0.5 * found[0].peak
        print(case, k, seed, found[0].peak, found[0].support)


def test_assemble_needs_neither_torch_nor_the_library():
    code = ("import sys; from porechop_amd.discover import assemble; assemble([], [], 8, 10); "
            "import porechop_amd._lib as L; assert 'torch' not in sys.modules and L._lib is None")
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---- rules --------------------------------------------------------------------------------------------------------------
def table_of(seq, k, count):
    """every k-mer of seq with `count` (an int, or one per k-mer)"""
    kmers = [seq[i:i + k] for i in range(len(seq) - k + 1)]
    counts = [count] * len(kmers) if isinstance(count, int) else list(count)
    assert len(counts) == len(kmers) and len(set(kmers)) == len(kmers)
    return [km.encode(x) for x in kmers], counts


def test_empty_candidate_list():
    assert assemble([], [], 8, 100) == []
    assert assemble(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 12, 0) == []
    codes, counts = table_of("ACGTTGCAAGGCTTAC", 8, 4)
    assert assemble(codes, counts, 8, 100) == []                   # below max(2, ceil(0.05 * 100)) = 5
    assert [f.sequence for f in assemble(codes, counts, 8, 80)] == ["ACGTTGCAAGGCTTAC"]      # ceil(4.0) = 4
    assert assemble(codes, [1] * len(codes), 8, 1) == []           # never below 2


def test_equal_counts_seed_from_the_lowest_code():
    a, b = "CCGTTGCAAGGCTTAC", "AGTCATGGACTTGACA"                  # two paths without a common k-mer, all counts equal
    ca, na = table_of(a, 8, 50)
    cb, nb = table_of(b, 8, 50)
    found = assemble(ca + cb, na + nb, 8, 100)
    # the lowest code of all is AAGGCTTA (inside a): a is found first, grown both ways from there
    assert min(ca + cb) == km.encode("AAGGCTTA")
    assert [f.sequence for f in found] == [a, b]
    assert all(f.peak == 50 and f.support == 50 for f in found)
    # the same table in another order
    rev = assemble((ca + cb)[::-1], (na + nb)[::-1], 8, 100)
    assert [f.sequence for f in rev] == [a, b]


def test_equal_successors_take_the_lowest_base():
    k = 6
    stem = "GATTACAGG"                                              # ends in k-mer TACAGG; successors ACAGG[ACGT]
    codes, counts = table_of(stem, k, [90, 90, 100, 90])
    for b in "TGC":                                                 # three equal successors, listed highest first
        codes.append(km.encode("ACAGG" + b))
        counts.append(60)
    found = assemble(codes, counts, k, 100, min_len=k)
    assert found[0].sequence == stem + "C"
    assert found[0].peak == 100 and found[0].support == 60
    # the others are left over as seeds of their own: equal counts, the lowest code first
    assert [f.sequence for f in found[1:]] == ["ACAGGG", "ACAGGT"]
    # ... and on the left: predecessors [ACGT]GATTA of GATTAC
    codes2, counts2 = table_of(stem, k, [90, 90, 100, 90])
    for b in "TG":
        codes2.append(km.encode(b + "GATTA"))
        counts2.append(70)
    assert assemble(codes2, counts2, k, 100, min_len=k)[0].sequence == "G" + stem


def test_homopolymer_terminates_and_is_dropped():
    k = 8
    found = assemble([km.encode("A" * k)], [1000], k, 100)
    assert found == []
    kept = assemble([km.encode("A" * k)], [1000], k, 100, min_len=1)
    assert [f.sequence for f in kept] == ["A" * k] and len(kept[0].sequence) <= k + 3
    # a two-k-mer cycle (ACACACAC <-> CACACACA) ends as well
    cyc = assemble([km.encode("AC" * 4), km.encode("CA" * 4)], [500, 500], k, 100, min_len=1)
    assert [f.sequence for f in cyc] == ["AC" * 4 + "A"]


def test_extend_ratio_stops_a_ramp_where_it_says():
    k = 6
    seq = "GATTACAGGCTTCA"                                          # 9 k-mers
    ramp = [30, 49, 50, 80, 100, 70, 50, 49, 30]                    # seed in the middle, falling to both sides
    codes, counts = table_of(seq, k, ramp)
    found = assemble(codes, counts, k, 100, extend_ratio=0.5, min_len=k)
    assert found[0].sequence == seq[2:12] == "TTACAGGCTT"   # k-mers 2..6: every count >= 50
    assert (found[0].peak, found[0].support) == (100, 50)
    # the ratio refers to the SEED's count, not to the neighbour's: 0.49 takes the 49s, 0.3 everything
    assert assemble(codes, counts, k, 100, extend_ratio=0.49, min_len=k)[0].sequence == seq[1:13]
    assert assemble(codes, counts, k, 100, extend_ratio=0.3, min_len=k)[0].sequence == seq
    assert assemble(codes, counts, k, 100, extend_ratio=1.0, min_len=k)[0].sequence == seq[4:4 + k]


def test_min_len_default_and_option():
    k = 6
    seq = "GATTACAGG"                                               # length k + 3
    codes, counts = table_of(seq, k, 40)
    assert assemble(codes, counts, k, 100) == []                   # default k + 4
    assert [f.sequence for f in assemble(codes, counts, k, 100, min_len=k + 3)] == [seq]
    codes, counts = table_of(seq + "C", k, 40)
    assert [f.sequence for f in assemble(codes, counts, k, 100)] == [seq + "C"]


# ---- FASTA and adapter sets -----------------------------------------------------------------------------------------------
def test_adapter_sets_pair_name_and_leave_known_out():
    d = Discovery(start=[Found("ACGTACGTAA", 9, 8), Found("AATGTACTTC", 9, 9, "SQK-NSK007_Y_Top", 100.0, True), Found("GGGTTTAAAC", 5, 5)],
                  end=[Found("TTGCATTGCA", 7, 6, "x", 60.0, False)], reads=10, windows=20, k=8)
    sets = d.adapter_sets()
    assert [(s.name, s.start, s.end) for s in sets] == [
        ("discovered_1", ("discovered_1_start", "ACGTACGTAA"), ("discovered_1_end", "TTGCATTGCA")),
        ("discovered_2", ("discovered_2_start", "GGGTTTAAAC"), None)]
    assert [s.name for s in d.adapter_sets(prefix="kit")] == ["kit_1", "kit_2"]
    only_end = Discovery(end=[Found("TTGCATTGCA", 7, 6)])
    assert [(s.name, s.start, s.end) for s in only_end.adapter_sets()] == [("discovered_1", None, ("discovered_1_end", "TTGCATTGCA"))]
    assert Discovery(start=[Found("AATGTACTTC", 9, 9, "n", 95.0, True)]).adapter_sets() == []


def test_fasta_round_trip(tmp_path):
    from porechop_amd.pipeline import AdapterSet
    sets = [AdapterSet("discovered_1", ("discovered_1_start", "ACGTACGTAA"), ("discovered_1_end", "TTGCATTGCA")),
            AdapterSet("discovered_2", ("discovered_2_start", "GGGTTTAAAC"), None),
            AdapterSet("my kit", None, ("my kit_end", "CCCCGGGGTTTT"))]
    path = dv.write_adapters(str(tmp_path / "a.fasta"), sets)
    assert open(path).read() == (">discovered_1_start\nACGTACGTAA\n>discovered_1_end\nTTGCATTGCA\n>discovered_2_start\nGGGTTTAAAC\n"
                                 ">my kit_end\nCCCCGGGGTTTT\n")
    assert dv.read_adapters(path) == sets
    assert dv.read_adapters(dv.write_adapters(str(tmp_path / "none.fasta"), [])) == []


def test_fasta_record_without_side_suffix_is_refused_by_name(tmp_path):
    path = tmp_path / "bad.fasta"
    path.write_text(">discovered_1_start\nACGT\n>my_primer\nACGTACGT\n")
    with pytest.raises(ValueError, match="my_primer"):
        dv.read_adapters(str(path))
    path.write_text(">_end\nACGT\n")
    with pytest.raises(ValueError, match="_end"):
        dv.read_adapters(str(path))


def test_discover_cli_keeps_the_main_cli_at_the_reference_option_set():
    from porechop_amd.__main__ import build_parser
    main_opts = {o for a in build_parser()._actions for o in a.option_strings}
    assert not main_opts & {"--k", "--min_fraction", "--extend_ratio", "--min_len", "--max_reads", "--adapters_out", "--extra_adapters"}


# ---- discover() and the command line over a stand-in aligner (the host logic; the census itself is tests/test_gpu_kmer_count.py's) ----
NEW_START, NEW_END = "GTCACGGAGATCCCCGTACGGGGTAGACCA", "AAAGGCATTTCCCTCCCATATAAG"


def model_aligner(oracle):
    """tests/cpu_aligner.py's oracle-backed stand-in plus the census from the model"""
    import torch
    from tests.cpu_aligner import OracleAligner

    class ModelAligner(OracleAligner):
        def kmer_count(self, arena, win_off, win_len, k, counts=None, stream=None):
            a = arena.numpy()
            windows = [a[o:o + n].tobytes() for o, n in zip(win_off.tolist(), win_len.tolist())]
            if counts is None:
                counts = torch.zeros(1 << (2 * k), dtype=torch.int32)
            counts += torch.from_numpy(km.count_dense(windows, k)).to(torch.int32)
            return counts

        def kmer_candidates(self, counts, k, min_count, cap=None):
            c = counts.numpy().astype(np.int64)
            codes = np.nonzero(c >= min_count)[0]
            order = np.lexsort((codes, -c[codes]))
            return codes[order], c[codes][order]

        def align_pairs(self, pairs, mode=0):
            out = np.zeros((len(pairs), 8), dtype=np.int32)
            for i, (rd, ai) in enumerate(pairs):
                r = self.oracle.align_raw(rd, self.adapters[ai].decode(), self.scores)
                out[i] = [-1, -1, -1, -1, 0, 0, 0, 0] if r.failed else [r.read_start, r.read_end, r.adapter_start, r.adapter_end, r.score,
                                                                        r.aligned_matches, r.aligned_len, r.full_len]
            return out

    return ModelAligner(oracle)


def write_fastq(path, reads):
    with open(path, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@read_%d\n%s\n+\n%s\n" % (i + 1, r, "5" * len(r)))
    return str(path)


def test_discover_annotates_pairs_and_feeds_the_runner(tmp_path, oracle, monkeypatch, capsys):
    from porechop_amd import runner
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import AdapterSet
    reads = km.planted_reads(1000, 0.8, 0.08, 7, NEW_START, NEW_END)
    path = write_fastq(tmp_path / "new.fastq", reads)
    d = dv.discover(path, aligner=model_aligner(oracle))
    assert (d.reads, d.windows, d.k) == (1000, 2000, 12)
    assert [f.sequence for f in d.start] == [NEW_START] and [f.sequence for f in d.end] == [NEW_END]
    assert all(f.nearest and f.identity < 70.0 and not f.known for f in d.start + d.end)
    sets = d.adapter_sets()
    assert sets == [AdapterSet("discovered_1", ("discovered_1_start", NEW_START), ("discovered_1_end", NEW_END))]
    # streamed: every block into the same pair of tables; max_reads stops the census
    monkeypatch.setenv("PC_STREAM_BLOCK_BYTES", "50000")
    again = dv.discover(path, aligner=model_aligner(oracle))
    assert (again.start, again.end, again.reads) == (d.start, d.end, d.reads)
    assert dv.discover(path, aligner=model_aligner(oracle), max_reads=300, min_len=100).reads == 300
    monkeypatch.delenv("PC_STREAM_BLOCK_BYTES")
    # the panel's own adapters come back known
    known = dv.discover(write_fastq(tmp_path / "known.fastq", km.planted_reads(1000, 0.8, 0.08, 8)), aligner=model_aligner(oracle))
    assert [(f.sequence, f.nearest, f.identity, f.known) for f in known.start] == [(km.Y_TOP, "SQK-NSK007_Y_Top", 100.0, True)]
    assert [(f.sequence, f.nearest, f.identity, f.known) for f in known.end] == [(km.Y_BOTTOM, "SQK-NSK007_Y_Bottom", 100.0, True)]
    assert known.adapter_sets() == []
    assert dv.report_lines(known)[0].split("\t")[5:] == ["SQK-NSK007_Y_Top", "100.0", "known"]
    # the run with the discovered sets trims; the default panel does not
    few = write_fastq(tmp_path / "few.fastq", reads[:150])
    out_a, out_b = str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq")
    runner.run(few, output=out_a, aligner=model_aligner(oracle), device="cpu")
    res = runner.run(few, output=out_b, aligner=model_aligner(oracle), device="cpu", adapter_panel=load_panel() + sets)
    assert res.matching_sets == ["discovered_1"]
    assert open(out_a).read() == open(few).read() and open(out_b).read() != open(few).read()
