"""Barcode discovery without a GPU: discover(barcodes=True) over the oracle-backed stand-in aligner of
tests/test_discover_host.py plus the numpy model of pc_anchor_inserts (tests/barcode_model.py) recovers planted barcodes
character for character; the rules of cluster_inserts and pair_barcodes on hand-made tables; Discovery.barcode_sets(), its
names and its FASTA; the main command line's option set."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import barcode_model as bm
from tests import kmer_model as km
from tests.test_discover_host import model_aligner, write_fastq

from porechop_amd import discover as dv
from porechop_amd.discover import AnchorInserts, BarcodeFound, Discovery, Found, cluster_inserts, pair_barcodes


def barcode_aligner(oracle):
    import torch
    base = model_aligner(oracle)

    class BarcodeModelAligner(type(base)):
        def anchor_inserts(self, arena, win_off, win_len, records, anchor_len, side, min_identity=75, insert_len=24, stream=None):
            return torch.from_numpy(bm.anchor_inserts(arena.numpy(), win_off.numpy(), win_len.numpy(), records.numpy(), anchor_len,
                                                      side, min_identity, insert_len))

    return BarcodeModelAligner(oracle)


# ---- planted recovery: the gate ------------------------------------------------------------------------------------------
GATE = [(3000, 12, 0.08, 1), (3000, 12, 0.08, 2), (3000, 12, 0.08, 3), (2000, 4, 0.08, 20), (2000, 4, 0.08, 21)]


def check_recovery(d, planted):
    """both sides exact and nothing else, the end barcodes the reverse complements, every pair right, everything new"""
    s, e = d.barcode_anchor("start"), d.barcode_anchor("end")
    assert s is not None and e is not None and (s.anchor, e.anchor) == (0, 0)       # the adapters themselves: found first
    assert sorted(f.sequence for f in s.barcodes) == sorted(planted)
    assert sorted(f.sequence for f in e.barcodes) == sorted(bm.rc(b) for b in planted)
    for i, f in enumerate(s.barcodes):
        assert f.partner is not None and e.barcodes[f.partner].sequence == bm.rc(f.sequence) and e.barcodes[f.partner].partner == i
        assert f.support >= f.peak >= 3 and not f.known
    assert not any(f.known for f in e.barcodes)
    sets = d.barcode_sets()
    assert [(x.start[1], x.end[1]) for x in sets] == [(f.sequence, bm.rc(f.sequence)) for f in s.barcodes]


@pytest.mark.parametrize("n,nb,e,seed", GATE)
def test_planted_barcodes_are_recovered_exactly(tmp_path, oracle, n, nb, e, seed):
    """The whole of discover(barcodes=True) over planted reads: both sides exact, no extra, all pairs right.

    Seeds 2 and 21 are the ones that need discover.trim_anchor: half or more of their barcodes begin with C (7 of 12; 2 of 4),
    so the census -- extend_ratio 0.5 -- returns the start adapter as A_S + "C" (seed 2: the end adapter as "G" + A_E too), and
    with that sequence as the anchor every barcode came back one base late, bc[1:] + flank[0] (seed 2:
    AAGCGGCACTTGTGAAGTGTTCCC for AAAGCGGCACTTGTGAAGTGTTCC, 12 of 12 so).  The found sequences are still reported that way;
    the anchors are A_S and A_E ("The anchor's inner edge")."""
    planted = bm.make_barcodes(nb, 24, seed)
    reads, _ = bm.barcoded_reads(n, planted, e, seed)
    path = write_fastq(tmp_path / "bc.fastq", reads)
    d = dv.discover(path, aligner=barcode_aligner(oracle), barcodes=True)
    for side in ("start", "end"):
        for a in d.barcodes[side]:
            print(side, a.anchor, a.sequence, a.anchored, [(f.sequence, f.peak, f.support) for f in a.barcodes], a.constant)
    print([f.sequence for f in d.start], [f.sequence for f in d.end])
    assert (d.barcode_anchor("start").anchor, d.barcode_anchor("end").anchor) == (0, 0)
    check_recovery(d, planted)
    # the adapters as the census reports them, one shared barcode base too long at times; the anchors without it
    assert d.start[0].sequence[:30] == bm.A_S and len(d.start[0].sequence) <= 31 and d.barcodes["start"][0].sequence == bm.A_S
    assert d.end[0].sequence[-24:] == bm.A_E and len(d.end[0].sequence) <= 25 and d.barcodes["end"][0].sequence == bm.A_E
    assert (seed not in (2, 21)) or d.start[0].sequence == bm.A_S + "C"


def test_streamed_max_reads_no_barcodes_and_the_option_off(tmp_path, oracle, monkeypatch):
    planted = bm.make_barcodes(4, 24, 5)
    reads, _ = bm.barcoded_reads(1200, planted, 0.08, 5)
    path = write_fastq(tmp_path / "bc.fastq", reads)
    whole = dv.discover(path, aligner=barcode_aligner(oracle), barcodes=True)
    check_recovery(whole, planted)
    plain = dv.discover(path, aligner=barcode_aligner(oracle))
    assert plain.barcodes == {} and plain.barcode_sets() == []
    assert (plain.start, plain.end, plain.reads) == (whole.start, whole.end, whole.reads)
    # after the pass the aligner holds the panel again: the found sequences are annotated as without it
    assert all(f.nearest is not None for f in whole.start + whole.end)
    monkeypatch.setenv("PC_STREAM_BLOCK_BYTES", "50000")
    streamed = dv.discover(path, aligner=barcode_aligner(oracle), barcodes=True)
    assert streamed == whole
    first = dv.discover(path, aligner=barcode_aligner(oracle), barcodes=True, max_reads=600)
    assert first.reads == 600 and sum(a.anchored for a in first.barcodes["start"][:1]) <= 600
    monkeypatch.delenv("PC_STREAM_BLOCK_BYTES")
    # planted adapters without barcodes: an anchor and nothing behind it
    none = dv.discover(write_fastq(tmp_path / "plain.fastq", km.planted_reads(1000, 0.8, 0.08, 7, bm.A_S, bm.A_E)),
                       aligner=barcode_aligner(oracle), barcodes=True)
    assert [f.sequence for f in none.start] == [bm.A_S] and [f.sequence for f in none.end] == [bm.A_E]
    assert [(a.anchor, a.barcodes, a.constant) for a in none.barcodes["start"] + none.barcodes["end"]] == [(0, [], None)] * 2
    assert none.barcodes["start"][0].anchored > 500 and none.barcode_sets() == [] and dv.barcode_report_lines(none) == []
    with pytest.raises(ValueError, match="barcode_len"):
        dv.discover(path, aligner=barcode_aligner(oracle), barcodes=True, barcode_len=32)
    with pytest.raises(ValueError, match="anchor_identity"):
        dv.discover(path, aligner=barcode_aligner(oracle), barcodes=True, anchor_identity=101)


def test_the_rule_needs_neither_torch_nor_the_library():
    code = ("import sys; from porechop_amd.discover import cluster_inserts, pair_barcodes; cluster_inserts([1, 2], [5, 5], 12, 10); "
            "pair_barcodes([], []); import porechop_amd._lib as L; assert 'torch' not in sys.modules and L._lib is None")
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---- the model of pc_anchor_inserts itself ---------------------------------------------------------------------------------
def test_model_of_anchor_inserts():
    arena = np.frombuffer(b"TTACGTNACGTACGTAA", dtype=np.uint8)
    rec = lambda rs, re_, a0, a1, m, full: [rs, re_, a0, a1, 0, m, full, full]
    off, ln = np.array([0, 0, 0, 0, 2], dtype=np.int64), np.array([17, 17, 17, 17, 4], dtype=np.int32)
    records = np.array([rec(0, 1, 0, 3, 4, 4), rec(0, 6, 0, 3, 4, 4), rec(-1, 0, 0, 0, 0, 0), rec(0, 2, 0, 3, 4, 4), rec(0, 1, 0, 3, 3, 4)],
                       dtype=np.int32)
    got = bm.anchor_inserts(arena, off, ln, records, 4, 0, 75, 4)
    #       ACGT behind column 1; ACGT behind the N; the failure record; CGTN holds a non-base; GT + 4 leaves the window
    assert got.tolist() == [km.encode("ACGT"), km.encode("ACGT"), -1, -1, -1]
    assert bm.anchor_inserts(arena, off[:1], ln[:1], np.array([rec(5, 8, 0, 3, 4, 4)]), 4, 1, 75, 4).tolist() == [km.encode("TACG")]
    assert bm.anchor_inserts(arena, off[:1], ln[:1], np.array([rec(3, 8, 0, 3, 4, 4)]), 4, 1, 75, 4).tolist() == [-1]      # col -1
    assert bm.anchor_inserts(arena, off[:1], ln[:1], np.array([rec(5, 8, 1, 3, 3, 4)]), 4, 1, 75, 4).tolist() == [-1]
    assert bm.anchor_inserts(arena, off[:1], ln[:1], np.array([rec(0, 1, 0, 2, 3, 4)]), 4, 0, 75, 4).tolist() == [-1]
    assert bm.anchor_inserts(arena, off[:1], ln[:1], np.array([rec(0, 1, 0, 3, 3, 4)]), 4, 0, 76, 4).tolist() == [-1]


# ---- cluster_inserts -----------------------------------------------------------------------------------------------------
L = 24


def rand_seq(rng, n=L):
    return "".join(rng.choice("ACGT") for _ in range(n))


def model_sd(a, b, max_shift=4):
    return min(min(bm.edit_distance(a[s:], b[:len(a) - s]), bm.edit_distance(b[s:], a[:len(a) - s])) for s in range(max_shift + 1))


def substituted(rng, seq, positions):
    out = list(seq)
    for p in positions:
        out[p] = rng.choice([b for b in "ACGT" if b != out[p]])
    return "".join(out)


def variant_at(rng, base, want):
    """a substitution variant of base whose shift distance to it is exactly `want`"""
    for _ in range(1000):
        v = substituted(rng, base, rng.sample(range(L), want))
        if model_sd(v, base) == want:
            return v
    raise AssertionError("no variant at distance %d" % want)


def test_distances_agree_with_the_plain_definition():
    rng = random.Random(11)
    assert dv.edit_distance("", "ACG") == 3 and dv.edit_distance("ACGT", "ACGT") == 0 and dv.edit_distance("ACGT", "AGT") == 1
    base = [rand_seq(rng) for _ in range(6)]
    rows = np.array([[km.encode(ch) for ch in b] for b in base])
    for _ in range(40):
        x = km.mutate(rng, rng.choice(base), 0.2)
        x = (x + rand_seq(rng))[:L] if rng.random() < 0.7 else (rand_seq(rng, 3) + x)[:L]
        want = [model_sd(x, b) for b in base]
        assert [dv.shift_distance(x, b) for b in base] == want
        assert dv._sd_to_all(np.array([km.encode(ch) for ch in x]), rows, 4).tolist() == want
        assert dv._sd_to_all(np.array([km.encode(ch) for ch in x]), rows, 0).tolist() == [bm.edit_distance(x, b) for b in base]


def test_floor():
    rng = random.Random(1)
    a, b, c = (km.encode(rand_seq(rng)) for _ in range(3))
    assert [f.peak for f in cluster_inserts([a, b, c], [3, 2, 40], L, 100)] == [40, 3]              # max(3, ceil(0.1)) = 3
    assert [f.peak for f in cluster_inserts([a, b, c], [3, 2, 40], L, 3001)] == [40]                # ceil(3.001) = 4
    assert [f.peak for f in cluster_inserts([a, b, c], [3, 2, 40], L, 3000)] == [40, 3]             # ceil(3.0) = 3
    assert [f.peak for f in cluster_inserts([a, b, c], [3, 2, 40], L, 100, min_count=2)] == [40, 3, 2]
    assert [f.peak for f in cluster_inserts([a, b, c], [3, 2, 40], L, 100, min_share=0.05)] == [40]
    assert cluster_inserts([], [], L, 0) == [] and cluster_inserts([a], [2], L, 10) == []
    assert dv.insert_floor(0) == 3 and dv.insert_floor(10 ** 6) == 1000


def test_order_and_ties():
    rng = random.Random(2)
    seqs = sorted(rand_seq(rng) for _ in range(4))                   # far apart: four centroids
    assert min(model_sd(x, y) for x in seqs for y in seqs if x != y) >= 5
    codes = [km.encode(s) for s in seqs]
    found = cluster_inserts(codes[::-1], [7, 9, 7, 9], L, 100)       # (codes listed highest first)
    # count descending, then code ascending (= the sequences' alphabetical order)
    assert [(f.sequence, f.peak, f.support) for f in found] == [(seqs[0], 9, 9), (seqs[2], 9, 9), (seqs[1], 7, 7), (seqs[3], 7, 7)]
    # a shadow of two centroids goes to the FIRST accepted one: base and far are 4 apart with min_dist 3, x is 2 from both
    base = seqs[0]
    far = substituted(rng, base, [2, 9, 15, 21])
    x = "".join(far[p] if p in (2, 9) else base[p] for p in range(L))
    assert (model_sd(base, far), model_sd(x, base), model_sd(x, far)) == (4, 2, 2)
    found = cluster_inserts([km.encode(s) for s in (far, base, x)], [20, 20, 5], L, 100, min_dist=3)
    first, second = sorted([base, far])
    assert [(f.sequence, f.peak, f.support) for f in found] == [(first, 20, 25), (second, 20, 20)]


def test_min_dist_edge():
    rng = random.Random(3)
    base = rand_seq(rng)
    near, at = variant_at(rng, base, 4), variant_at(rng, base, 5)
    assert model_sd(near, at) >= 5                                    # (so `at` is judged against base alone)
    found = cluster_inserts([km.encode(s) for s in (base, near, at)], [100, 10, 9], L, 500)
    assert [(f.sequence, f.peak, f.support) for f in found] == [(base, 100, 110), (at, 9, 9)]
    found = cluster_inserts([km.encode(s) for s in (base, near, at)], [100, 10, 9], L, 500, min_dist=6)
    assert [(f.sequence, f.peak, f.support) for f in found] == [(base, 100, 119)]
    found = cluster_inserts([km.encode(s) for s in (base, near, at)], [100, 10, 9], L, 500, min_dist=4)
    assert [(f.sequence, f.peak, f.support) for f in found] == [(base, 100, 100), (near, 10, 10), (at, 9, 9)]


def test_a_shifted_copy_is_merged():
    rng = random.Random(4)
    for shift in (1, 2, 3, 4):
        base = rand_seq(rng)
        late = base[shift:] + rand_seq(rng, shift)                    # the insert taken `shift` bases late
        early = rand_seq(rng, shift) + base[:L - shift]
        assert model_sd(late, base) == 0 and model_sd(early, base) == 0
        found = cluster_inserts([km.encode(s) for s in (base, late, early)], [100, 8, 6], L, 500)
        assert [(f.sequence, f.peak, f.support) for f in found] == [(base, 100, 114)]
    # by 3: the plain edit distance is at or above min_dist, and without the shift tolerance the copy is a false barcode
    base = rand_seq(rng)
    late = base[3:] + rand_seq(rng, 3)
    assert bm.edit_distance(late, base) >= 5
    assert [f.sequence for f in cluster_inserts([km.encode(base), km.encode(late)], [100, 8], L, 500, max_shift=0)] == [base, late]
    assert [f.sequence for f in cluster_inserts([km.encode(base), km.encode(late)], [100, 8], L, 500)] == [base]
    # the tolerance ends: a copy shifted by 7 is 3 bases beyond max_shift = 4, about 6 edits
    beyond = base[7:] + rand_seq(rng, 7)
    assert model_sd(beyond, base) >= 5
    assert len(cluster_inserts([km.encode(base), km.encode(beyond)], [100, 8], L, 500)) == 2


def test_other_insert_lengths():
    rng = random.Random(6)
    for n in (1, 12, 31):
        a = rand_seq(rng, n)
        b = "".join("ACGT"[("ACGT".index(ch) + 1) % 4] for ch in a)  # every base different: far at n >= 12
        found = cluster_inserts([km.encode(a), km.encode(b)], [10, 9], n, 50, min_dist=1)
        assert [f.sequence for f in found] == [a, b]


# ---- trim_anchor ---------------------------------------------------------------------------------------------------------
def test_an_anchor_is_trimmed_where_its_edge_base_is_not_common():
    k = 6
    seq = "GATTACAGGCTTCA"                                            # 9 k-mers
    kmers = [seq[i:i + k] for i in range(len(seq) - k + 1)]

    def table(counts):
        t = dict(zip((km.encode(x) for x in kmers), counts))
        return lambda code: t.get(code, 0)
    level = [100] * 9
    assert dv.trim_anchor(seq, 0, table(level), k) == seq and dv.trim_anchor(seq, 1, table(level), k) == seq
    # the start side's inner edge is the right end: 89 of 100 is below 0.9, 90 is not
    assert dv.trim_anchor(seq, 0, table([100] * 8 + [89]), k) == seq[:-1]
    assert dv.trim_anchor(seq, 0, table([100] * 8 + [90]), k) == seq
    assert dv.trim_anchor(seq, 0, table([100] * 8 + [74]), k, edge_ratio=0.7) == seq
    # base after base, each against the k-mer before it, until one holds; the outer edge is never looked at
    assert dv.trim_anchor(seq, 0, table([30, 100, 100, 100, 100, 100, 100, 58, 30]), k) == seq[:-2]
    assert dv.trim_anchor(seq, 0, table([30, 100, 100, 100, 100, 100, 100, 95, 30]), k) == seq[:-1]
    # the end side's inner edge is the left end
    assert dv.trim_anchor(seq, 1, table([74] + [100] * 8), k) == seq[1:]
    assert dv.trim_anchor(seq, 1, table([30, 58, 100, 100, 100, 100, 100, 100, 30]), k) == seq[2:]
    assert dv.trim_anchor(seq, 1, table([100] * 8 + [10]), k) == seq
    # never below k bases, whatever the counts
    assert dv.trim_anchor(seq, 0, table([1000, 500, 250, 120, 60, 30, 15, 7, 3]), k) == seq[:k]
    assert dv.trim_anchor(seq[:k], 0, table(level), k) == seq[:k]


# ---- pair_barcodes -------------------------------------------------------------------------------------------------------
def centroids(seqs):
    return [BarcodeFound(s, 10, 10) for s in seqs]


def test_pairing_by_reverse_complement():
    rng = random.Random(7)
    a, b, c = (rand_seq(rng) for _ in range(3))
    start, end = centroids([a, b, c]), centroids([bm.rc(c), rand_seq(rng), bm.rc(a)])
    assert pair_barcodes(start, end) == [(0, 2), (2, 0)]
    assert [f.partner for f in start] == [2, None, 0] and [f.partner for f in end] == [2, None, 0]
    # the rule comes first: co-occurrence counts that say otherwise do not undo it
    sc = np.array([km.encode(a)] * 5, dtype=np.int64)
    ec = np.array([km.encode(end[1].sequence)] * 5, dtype=np.int64)
    assert pair_barcodes(start, end, sc, ec) == [(0, 2), (2, 0)]


def test_pairing_by_mutual_best_co_occurrence_and_a_tie():
    rng = random.Random(8)
    s = [rand_seq(rng) for _ in range(3)]
    e = [rand_seq(rng) for _ in range(3)]
    start, end = centroids(s), centroids(e)

    def reads(*triples):
        sc, ec = [], []
        for i, j, n in triples:
            sc += [km.encode(s[i]) if i is not None else -1] * n
            ec += [km.encode(e[j]) if j is not None else -1] * n
        return np.array(sc + [12345, -1], dtype=np.int64), np.array(ec + [-1, 54321], dtype=np.int64)
    # 0 <-> 1 mutual best; start 1's best is end 1 as well, but end 1 prefers start 0; start 2 and end 2 meet once only
    assert pair_barcodes(start, end, *reads((0, 1, 6), (1, 1, 4), (1, 0, 3), (2, 2, 1), (0, None, 9))) == [(0, 1)]
    assert [f.partner for f in start] == [1, None, None] and [f.partner for f in end] == [None, 0, None]
    # ... with a second read they pair; start 1 still prefers end 1 and stays alone, until those reads are gone
    assert pair_barcodes(start, end, *reads((0, 1, 6), (1, 1, 4), (1, 0, 3), (2, 2, 2))) == [(0, 1), (2, 2)]
    assert pair_barcodes(start, end, *reads((0, 1, 6), (1, 0, 3), (2, 2, 2))) == [(0, 1), (1, 0), (2, 2)]
    # a tie goes to the lowest index on either side: start 0 sees ends 0 and 1 equally often and end 0 sees starts 0 and 1
    # equally often -> (0, 0); start 1's best, end 0, is taken, and end 1's best, start 0, as well
    assert pair_barcodes(start, end, *reads((0, 0, 3), (0, 1, 3), (1, 0, 3))) == [(0, 0)]
    # start 1 sees ends 0 and 1 equally often -> end 0, whose only start it is; end 1 sees starts 0 and 1 -> start 0, whose only end it is
    assert pair_barcodes(start, end, *reads((0, 1, 3), (1, 0, 3), (1, 1, 3))) == [(0, 1), (1, 0)]
    assert pair_barcodes(start, end) == [] and pair_barcodes([], end) == []


# ---- barcode_sets, names, FASTA ------------------------------------------------------------------------------------------
def made_discovery():
    rng = random.Random(9)
    a, b, c, d = (rand_seq(rng) for _ in range(4))
    start = [BarcodeFound(a, 30, 40, partner=1), BarcodeFound(b, 28, 30, partner=None),
             BarcodeFound(c, 20, 22, partner=0, nearest="BC01", identity=95.8, known=True), BarcodeFound(d, 9, 9, partner=2)]
    end = [BarcodeFound(bm.rc(c), 19, 20, partner=2), BarcodeFound(bm.rc(a), 29, 33, partner=0), BarcodeFound(bm.rc(d), 9, 9, partner=3),
           BarcodeFound(rand_seq(rng), 5, 5)]
    disc = Discovery(start=[Found("ACGTACGTACGTACGTAA", 50, 40), Found(bm.A_S, 90, 80)], end=[Found(bm.A_E, 88, 80)], reads=100, windows=200,
                     barcodes={"start": [AnchorInserts(0, 70, constant=BarcodeFound(rand_seq(rng), 60, 66)), AnchorInserts(1, 120, start)],
                               "end": [AnchorInserts(0, 110, end)]})
    return disc, (a, b, c, d)


def test_barcode_sets_names_and_known_left_out(tmp_path):
    from porechop_amd import panel
    from porechop_amd.pipeline import AdapterSet
    disc, (a, b, c, d) = made_discovery()
    sets = disc.barcode_sets()
    n1, n2, n4 = ("Barcode discovered_%d (forward)" % i for i in (1, 2, 4))
    assert sets == [AdapterSet(n1, (n1 + "_start", a), (n1 + "_end", bm.rc(a))), AdapterSet(n2, (n2 + "_start", b), None),
                    AdapterSet(n4, (n4 + "_start", d), (n4 + "_end", bm.rc(d)))]           # 3 is known; the end-only centroid is not emitted
    assert [s.name for s in disc.barcode_sets(prefix="kit")] == ["Barcode kit_1 (forward)", "Barcode kit_2 (forward)", "Barcode kit_4 (forward)"]
    for s in sets:
        assert panel.is_barcode(s) and panel.barcode_direction(s) == "forward" and panel.phase_b_pair_key(s) is None
        assert panel.barcode_name(s) == s.name.replace(" ", "_")
    assert panel.choose_barcoding_kit(sets, lambda s: 95.0, lambda s: 0.0) == "forward"
    assert len(set(panel.barcode_name(s) for s in sets)) == 3
    # the FASTA of sets carries them unchanged, beside adapter sets
    both = disc.adapter_sets() + sets
    path = dv.write_adapters(str(tmp_path / "sets.fasta"), both)
    assert dv.read_adapters(path) == both
    assert ">Barcode discovered_1 (forward)_start\n%s\n>Barcode discovered_1 (forward)_end\n%s\n" % (a, bm.rc(a)) in open(path).read()
    # the report: one line per barcode, the constant continuation said to be one
    lines = [x.split("\t") for x in dv.barcode_report_lines(disc)]
    assert [x[0] for x in lines] == ["start"] * 5 + ["end"] * 4 and [x[1] for x in lines] == ["0", "1", "1", "1", "1", "0", "0", "0", "0"]
    assert lines[0][7] == "constant" and lines[1] == ["start", "1", a, "30", "40", "%.4f" % (40 / 120), "1", "new"]
    assert lines[3][6:] == ["0", "known"] and lines[8][6:] == ["-", "new"]
    assert Discovery().barcode_sets() == [] and dv.barcode_report_lines(Discovery()) == []


def test_discover_cli_keeps_the_main_cli_at_the_reference_option_set():
    from porechop_amd.__main__ import build_parser
    main_opts = {o for a in build_parser()._actions for o in a.option_strings}
    assert not main_opts & {"--barcodes", "--barcode_len", "--anchor_identity", "--barcode_min_share", "--barcode_min_count", "--barcode_min_dist", "--anchor_edge_ratio"}
