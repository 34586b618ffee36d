"""Barcode discovery end to end on the MI355X: 3000 reads carry one of 12 planted barcodes between two adapters no panel knows;
discover(barcodes=True) returns the barcodes and their reverse complements character for character, paired and marked new, a
binning run with the discovered sets writes the files a run with the true sequences writes, and the command line does the same
in one go."""
import os

import pytest

from tests import barcode_model as bm
from tests import kmer_model as km

pytestmark = pytest.mark.gpu

SEED, NB = 1, 12


def write_fastq(path, reads):
    with open(path, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@read_%d\n%s\n+\n%s\n" % (i + 1, r, "5" * len(r)))
    return str(path)


def files_of(directory):
    return {f: open(os.path.join(directory, f), "rb").read() for f in sorted(os.listdir(directory))}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("barcodes")
    barcodes = bm.make_barcodes(NB, 24, SEED)
    reads, which = bm.barcoded_reads(3000, barcodes, 0.08, SEED)
    return d, write_fastq(d / "bc.fastq", reads), reads, barcodes, which


@pytest.fixture(scope="module")
def discovery(planted):
    from porechop_amd.discover import discover
    return discover(planted[1], barcodes=True)


def test_the_planted_barcodes_come_back_exactly(planted, discovery):
    from porechop_amd.discover import discover
    d, barcodes = discovery, planted[3]
    for side in ("start", "end"):
        for a in d.barcodes[side]:
            print(side, a.anchor, a.anchored, [(f.sequence, f.peak, f.support, f.partner) for f in a.barcodes], a.constant)
    # the adapters are found as before, and without the option the result is today's
    plain = discover(planted[1])
    assert (plain.start, plain.end, plain.reads, plain.windows, plain.k) == (d.start, d.end, 3000, 6000, 12)
    assert plain.barcodes == {} and plain.barcode_sets() == []
    assert [f.sequence for f in d.start] == [bm.A_S] and [f.sequence for f in d.end] == [bm.A_E]
    assert not any(f.known for f in d.start + d.end)
    # both sides exact and nothing else
    assert [(a.anchor, len(a.barcodes)) for a in d.barcodes["start"]] == [(0, NB)] and [(a.anchor, len(a.barcodes)) for a in d.barcodes["end"]] == [(0, NB)]
    s, e = d.barcodes["start"][0], d.barcodes["end"][0]
    assert sorted(f.sequence for f in s.barcodes) == sorted(barcodes)
    assert sorted(f.sequence for f in e.barcodes) == sorted(bm.rc(b) for b in barcodes)
    assert 0.7 * 3000 < s.anchored <= 3000 and 0.7 * 3000 < e.anchored <= 3000
    for i, f in enumerate(s.barcodes):
        assert e.barcodes[f.partner].sequence == bm.rc(f.sequence) and e.barcodes[f.partner].partner == i
    for f in s.barcodes + e.barcodes:
        assert f.support >= f.peak >= 3 and f.nearest is not None and 0.0 <= f.identity < 90.0 and not f.known
    sets = d.barcode_sets()
    assert [x.name for x in sets] == ["Barcode discovered_%d (forward)" % (i + 1) for i in range(NB)]
    assert [(x.start, x.end) for x in sets] == [((x.name + "_start", f.sequence), (x.name + "_end", bm.rc(f.sequence)))
                                                 for x, f in zip(sets, s.barcodes)]


def test_a_streamed_run_returns_the_same(planted, discovery, monkeypatch):
    from porechop_amd import discover as dv
    from porechop_amd import io
    monkeypatch.setenv("PC_STREAM_BLOCK_BYTES", "100000")
    blocks = []
    real = io.ReadSet.segment
    monkeypatch.setattr(io.ReadSet, "segment", staticmethod(lambda p, b, t: (blocks.append(b), real(p, b, t))[1]))
    d = dv.discover(planted[1], barcodes=True)
    assert len(blocks) > 10                                            # (both passes, more than five blocks each)
    assert d == discovery


def test_a_binning_run_with_the_discovered_sets_equals_one_with_the_true_sequences(planted, discovery):
    from porechop_amd import runner
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import AdapterSet
    d, path, reads, barcodes, which = planted
    found = discovery.adapter_sets() + discovery.barcode_sets()
    # the TRUE sequences under the same set names: set i is the planted barcode its start sequence was found to be
    number = {s.start[1]: s.name for s in discovery.barcode_sets()}
    truth = [AdapterSet("discovered_1", ("discovered_1_start", bm.A_S), ("discovered_1_end", bm.A_E))]
    truth += sorted((AdapterSet(number[b], (number[b] + "_start", b), (number[b] + "_end", bm.rc(b))) for b in barcodes),
                    key=lambda s: int(s.name.split("_")[1].split()[0]))
    got_dir, want_dir = str(d / "bins_found"), str(d / "bins_truth")
    res = runner.run(path, barcode_dir=got_dir, adapter_panel=load_panel() + found)
    runner.run(path, barcode_dir=want_dir, adapter_panel=load_panel() + truth)
    assert res.matching_sets[0] == "discovered_1" and len(res.matching_sets) == 1 + NB
    got, want = files_of(got_dir), files_of(want_dir)
    assert got == want
    bins = ["Barcode_discovered_%d_(forward).fastq" % (i + 1) for i in range(NB)]
    assert sorted(got) == sorted(bins + ["none.fastq"]) and all(len(got[b]) > 0 for b in bins)
    # the reads are where their barcodes say: 96 % of them carry the barcode on at least one end (f = 0.8 per end), and a call
    # needs 75 % of it.  (A read in another barcode's bin is the demultiplexer's business -- a chance match in a read that
    # carries none -- and is printed, not judged.)
    right = wrong = 0
    for b in bins:
        for header in got[b].decode().split("\n")[0::4]:
            if header:
                i = int(header[1:].split()[0].split("_")[1]) - 1
                own = number[barcodes[which[i]]].replace(" ", "_") + ".fastq"
                right, wrong = right + (own == b), wrong + (own != b)
    print(right, wrong)
    assert right > 0.85 * 3000


def test_the_default_panel_bins_nothing(planted):
    """No set of the default panel is on these reads: a trimming run leaves them as they are, and a binning run ends where the
    reference's ends when no barcode set matches (porechop.py:343-366), before any file is written."""
    from porechop_amd import runner
    d, path, reads = planted[:3]
    out = str(d / "default.fastq")
    runner.run(path, output=out)
    lines = open(out).read().split("\n")
    assert lines[1::4] == reads
    with pytest.raises(runner.UsageError, match="no barcodes were found"):
        runner.run(path, barcode_dir=str(d / "bins_default"))
    assert not os.path.isdir(str(d / "bins_default")) or os.listdir(str(d / "bins_default")) == []


def test_command_line(planted, discovery, capsys):
    from porechop_amd import discover as dv
    d, path = planted[:2]
    fasta, got_dir = str(d / "cli.fasta"), str(d / "bins_cli")
    dv.main(["-i", path, "--barcodes", "--adapters_out", fasta, "-b", got_dir])
    printed = capsys.readouterr().out
    assert "start\t%s\t" % bm.A_S in printed and "end\t%s\t" % bm.A_E in printed
    assert "side\tanchor\tbarcode\tpeak\tsupport\tshare\tpartner\tstatus" in printed
    for i, f in enumerate(discovery.barcodes["start"][0].barcodes):
        assert "start\t0\t%s\t%d\t%d\t" % (f.sequence, f.peak, f.support) in printed
        assert "end\t0\t%s\t" % bm.rc(f.sequence) in printed
    assert printed.count("\tnew") == 2 + 2 * NB
    assert dv.read_adapters(fasta) == discovery.adapter_sets() + discovery.barcode_sets()
    assert files_of(got_dir) == files_of(str(d / "bins_found"))       # (the run of the test above)
    # without --barcodes the table and the FASTA are what they were
    plain = str(d / "plain.fasta")
    dv.main(["-i", path, "--adapters_out", plain])
    printed = capsys.readouterr().out
    assert "anchor" not in printed and printed.count("\n") == 3
    assert dv.read_adapters(plain) == discovery.adapter_sets()


def test_reads_without_barcodes_report_none(planted):
    from porechop_amd.discover import barcode_report_lines, discover
    path = write_fastq(planted[0] / "plain.fastq", km.planted_reads(3000, 0.8, 0.08, 7, bm.A_S, bm.A_E))
    d = discover(path, barcodes=True)
    assert [f.sequence for f in d.start] == [bm.A_S] and [f.sequence for f in d.end] == [bm.A_E]
    for side in ("start", "end"):
        assert [(a.anchor, a.barcodes, a.constant) for a in d.barcodes[side]] == [(0, [], None)]
        assert d.barcodes[side][0].anchored > 0.7 * 0.8 * 3000
    assert d.barcode_sets() == [] and barcode_report_lines(d) == []
    assert d.adapter_sets() == discover(path).adapter_sets()
