"""Adapter discovery end to end on the MI355X: two adapters no panel knows are planted in a FASTQ file, discover() returns
them character for character and marks them new, a run with the discovered sets trims exactly what a run with the true
strings trims; the panel's own adapters come back as known; the command line does the same in one go."""
import pytest

from tests import kmer_model as km

pytestmark = pytest.mark.gpu

# two fixed random strings; test_discovery_finds_the_planted_strings asserts through discover()'s own annotation that no
# panel sequence comes within 70 % of either
NEW_START, NEW_END = "GTCACGGAGATCCCCGTACGGGGTAGACCA", "AAAGGCATTTCCCTCCCATATAAG"


def write_fastq(path, reads):
    with open(path, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@read_%d\n%s\n+\n%s\n" % (i + 1, r, "5" * len(r)))
    return str(path)


def read_fastq(path):
    lines = open(path).read().split("\n")
    return dict(zip((x[1:] for x in lines[0::4]), lines[1::4]))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("discover")
    reads = km.planted_reads(3000, 0.8, 0.08, 7, NEW_START, NEW_END)
    return d, write_fastq(d / "new.fastq", reads), reads


@pytest.fixture(scope="module")
def discovery(planted):
    from porechop_amd.discover import discover
    return discover(planted[1])


def test_discovery_finds_the_planted_strings(discovery):
    d = discovery
    assert (d.reads, d.windows, d.k) == (3000, 6000, 12)
    assert [f.sequence for f in d.start] == [NEW_START]
    assert [f.sequence for f in d.end] == [NEW_END]
    for f in d.start + d.end:
        print(f)
        assert f.nearest is not None and 0.0 <= f.identity < 70.0 and not f.known
        assert f.peak >= f.support >= 0.5 * f.peak and f.support >= 0.05 * d.reads
    sets = d.adapter_sets()
    assert [(s.name, s.start, s.end) for s in sets] == [
        ("discovered_1", ("discovered_1_start", NEW_START), ("discovered_1_end", NEW_END))]


def test_streamed_blocks_fill_the_same_tables(planted, discovery, monkeypatch):
    from porechop_amd import discover as dv
    from porechop_amd import io
    monkeypatch.setenv("PC_STREAM_BLOCK_BYTES", "100000")
    blocks = []
    real = io.ReadSet.segment
    monkeypatch.setattr(io.ReadSet, "segment", staticmethod(lambda p, b, t: (blocks.append(b), real(p, b, t))[1]))
    d = dv.discover(planted[1])
    assert len(blocks) > 5
    assert (d.start, d.end, d.reads) == (discovery.start, discovery.end, discovery.reads)
    first = dv.discover(planted[1], max_reads=1000)
    assert first.reads == 1000 and [f.sequence for f in first.start] == [NEW_START]


def test_a_run_with_the_discovered_sets_equals_a_run_with_the_true_strings(planted, discovery):
    from porechop_amd import runner
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import AdapterSet
    d, path, reads = planted
    out = {x: str(d / ("out_%s.fastq" % x)) for x in "abc"}
    runner.run(path, output=out["a"])
    runner.run(path, output=out["b"], adapter_panel=load_panel() + discovery.adapter_sets())
    truth = AdapterSet("discovered_1", ("discovered_1_start", NEW_START), ("discovered_1_end", NEW_END))
    res = runner.run(path, output=out["c"], adapter_panel=load_panel() + [truth])
    assert res.matching_sets == ["discovered_1"]
    a = read_fastq(out["a"])
    assert a == {"read_%d" % (i + 1): r for i, r in enumerate(reads)}             # the default panel trims nothing
    b, c = open(out["b"], "rb").read(), open(out["c"], "rb").read()
    assert b == c and b != open(out["a"], "rb").read()
    assert sum(map(len, read_fastq(out["b"]).values())) < sum(map(len, reads)) - 20 * len(reads)


def test_the_panels_own_adapters_are_reported_known(planted):
    from porechop_amd.discover import discover
    d = planted[0]
    path = write_fastq(d / "known.fastq", km.planted_reads(3000, 0.8, 0.08, 8))
    found = discover(path)
    assert [(f.sequence, f.nearest, f.identity, f.known) for f in found.start] == [(km.Y_TOP, "SQK-NSK007_Y_Top", 100.0, True)]
    assert [(f.sequence, f.nearest, f.identity, f.known) for f in found.end] == [(km.Y_BOTTOM, "SQK-NSK007_Y_Bottom", 100.0, True)]
    assert found.adapter_sets() == []


def test_command_line(planted, discovery, capsys):
    from porechop_amd import discover as dv
    from porechop_amd import runner
    from porechop_amd.panel import load_panel
    d, path, _ = planted
    fasta, out, want = str(d / "cli.fasta"), str(d / "cli.fastq"), str(d / "cli_want.fastq")
    dv.main(["-i", path, "--adapters_out", fasta, "-o", out])
    printed = capsys.readouterr().out
    assert "start\t%s\t" % NEW_START in printed and "end\t%s\t" % NEW_END in printed and "\tnew" in printed
    assert dv.read_adapters(fasta) == discovery.adapter_sets()
    runner.run(path, output=want, adapter_panel=load_panel() + discovery.adapter_sets())
    assert open(out, "rb").read() == open(want, "rb").read()
    # --extra_adapters: the FASTA of one run is the panel extension of the next (--min_len 100: this one finds nothing itself)
    again = str(d / "cli2.fastq")
    dv.main(["-i", path, "--extra_adapters", fasta, "--min_len", "100", "-o", again])
    assert capsys.readouterr().out.split("\n")[1].startswith("3000 reads")
    assert open(again, "rb").read() == open(want, "rb").read()
