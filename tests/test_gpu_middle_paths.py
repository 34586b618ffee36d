"""Paths of middle hits on the MI355X (pc_middle_paths / Aligner.middle_paths, Pipeline.middle_hit_paths and the report
column built on them).

Kernel level: the hits of tests/middlegen.py -- about 170 per scheme, found on the host by a restatement of the
mask-and-realign loop over the C oracle, in reads of 1 to 1 920 bases at odd byte offsets of one arena, adapters of 1, 8, 9,
28, 33 and 111 bases mixed within every wave, reads with three and four hits, hits at column 1, cut by the read's end, and
in the interior of reads longer than window + W -- under the default, a linear, an open-above-extend and a refused scheme.
The expected values are Aligner.align_pairs_paths over the explicitly masked WHOLE read: records, heads and decoded
operations must be equal for every hit, and each path must pass tests/pathcheck.py on the masked string.

Pipeline and runner: a seeded batch of short reads with planted chimeras through phase_c's three routes, and the report
column middle_cigars of a whole and a streamed run."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import middlegen as mg
from tests import pathcheck

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN = mg.LONG


@pytest.fixture(scope="module")
def cases(oracle):
    return mg.Cases(oracle)


@pytest.fixture(scope="module")
def aligners(cases):
    import porechop_amd
    made = {}

    def get(name):
        if name not in made:
            made[name] = porechop_amd.Aligner(cases.adapters, mg.SCHEMES[name])
        return made[name]
    yield get
    for al in made.values():
        al.close()


def device_inputs(cases, hits):
    """The arguments of Aligner.middle_paths for a hit list, on the device."""
    import torch
    from porechop_amd.pipeline import middle_mask_tables
    t = lambda xs, dt: torch.tensor(xs, dtype=dt, device="cuda")
    arena = torch.from_numpy(np.frombuffer(cases.arena, dtype=np.uint8).copy()).cuda()
    read = t([h.read for h in hits], torch.int64)
    intervals, base, count = middle_mask_tables(read, t([h.start for h in hits], torch.int32), t([h.end for h in hits], torch.int32))
    return dict(arena=arena, read_off=t([cases.off[h.read] for h in hits], torch.int64),
                read_len=t([cases.length[h.read] for h in hits], torch.int32), adapter_idx=t([h.adapter for h in hits], torch.int32),
                read_end=t([h.end for h in hits], torch.int32), mask_base=base, mask_count=count, intervals=intervals)


def run(al, inputs):
    from porechop_amd.batch import decode_paths
    recs, heads, ops = al.middle_paths(max_len=MAX_LEN, **inputs)
    al.sync()
    n = int(inputs["read_off"].shape[0])
    assert tuple(recs.shape) == (n, 8) and tuple(heads.shape) == (n, 4) and int(ops.shape[0]) == n
    recs, heads, ops = recs.cpu().numpy(), heads.cpu().numpy(), ops.cpu().numpy()
    return recs, heads, ops, decode_paths(heads, ops)


_expected = {}


def expected(al, cases, name):
    """align_pairs_paths over the explicitly masked whole reads, once per scheme."""
    if name not in _expected:
        _expected[name] = al.align_pairs_paths([(h.masked, h.adapter) for h in cases.hits(name)])
    return _expected[name]


def test_the_cases_are_the_ones_asked_for(cases):
    from collections import Counter
    hits = cases.hits("default")
    assert 150 <= len(hits) <= 260
    assert {len(cases.adapters[h.adapter]) for h in hits} == set(mg.ADAPTER_LENGTHS)
    for w in range(0, len(hits) - 63, 64):                                  # mixed within every wave
        assert len({h.adapter for h in hits[w:w + 64]}) >= 4
    per_read = Counter(h.read for h in hits)
    three = [r for r, k in per_read.items() if k >= 3]
    assert len(three) >= 5
    assert any(len({h.adapter for h in hits if h.read == r}) < per_read[r] for r in three)       # the same adapter twice
    assert any(h.start == 0 for h in hits) and any(h.end == cases.length[h.read] for h in hits)
    # the interior of a read longer than window + W (c0 > 0 and c1 < n), for the 28-mer (W 70, window 174) and the 111-mer
    # (W 277, window 671)
    for a, W, window in ((3, 70, 174), (5, 277, 671)):
        assert any(h.adapter == a and h.end > window and h.end + W < cases.length[h.read] for h in hits), a
    assert any(h.rank >= 2 for h in hits) and min(cases.length) == 1 and max(cases.length) == mg.LONG
    reads = [h.read for h in hits]
    assert reads != sorted(reads)                                           # the reads interleave across rounds


@pytest.mark.parametrize("name", list(mg.SCHEMES))
def test_every_hit_of_every_scheme(cases, aligners, oracle, name):
    al = aligners(name)
    hits = cases.hits(name)
    assert len(hits) >= 150
    want_recs, want_heads, want_strings = expected(al, cases, name)
    recs, heads, ops, strings = run(al, device_inputs(cases, hits))
    for k, h in enumerate(hits):
        where = (name, k, h.read, h.adapter, h.start, h.end, h.rank)
        assert recs[k].tolist() == want_recs[k].tolist() and heads[k].tolist() == want_heads[k].tolist(), where
        assert strings[k] == want_strings[k], where
        assert (int(recs[k][0]), int(recs[k][1]) + 1) == (h.start, h.end), where
        try:
            pathcheck.check_path(h.masked, cases.adapters[h.adapter], mg.SCHEMES[name], recs[k], heads[k], strings[k],
                                 oracle.align_raw(h.masked, cases.adapters[h.adapter], mg.SCHEMES[name]))
        except AssertionError as e:
            raise AssertionError("%r: %s" % (where, e))
    # the data exercises something: gapped paths under every scheme, mismatches where a mismatch costs less than two gap
    # steps (under open_above_extend no optimal path holds an X)
    assert any("I" in s or "D" in s for s in strings)
    assert name == "open_above_extend" or any("X" in s for s in strings)


@pytest.mark.parametrize("count", [0, 1, 63, 65])
def test_hit_counts(cases, aligners, count):
    """n == 0 and hit counts that are no multiple of 64.  (The first `count` hits are all of round 0: no masks; the expected
    values are the whole list's.)"""
    al = aligners("default")
    hits = cases.hits("default")[:count]
    assert all(h.rank == 0 for h in hits)
    want_recs, want_heads, want_strings = expected(al, cases, "default")
    recs, heads, ops, strings = run(al, device_inputs(cases, hits))
    assert recs.tolist() == want_recs[:count].tolist() and heads.tolist() == want_heads[:count].tolist()
    assert strings == want_strings[:count]


def test_slices_give_what_one_launch_gives(cases, aligners, monkeypatch):
    al = aligners("default")
    inputs = device_inputs(cases, cases.hits("default"))
    n = len(cases.hits("default"))
    whole = run(al, inputs)
    # pc_align_paths' rule over this kernel's scratch: widest window (948 columns: the 111-mer's window + W) * row groups of the
    # longest adapter * 4 bytes per hit; a launch never holds fewer than 64 hits
    cols = al.middle_paths_cols(MAX_LEN)
    assert cols == 948
    per_hit = cols * ((111 + 7) // 8) * 4
    launch = max(64, ((1 << 20) // per_hit) // 64 * 64)
    assert -(-n // launch) >= 3
    monkeypatch.setenv("PC_PATHS_SCRATCH_MB", "1")
    sliced = run(al, inputs)
    for a, b in zip(whole[:3], sliced[:3]):
        assert np.array_equal(a, b)


def test_widest_window_on_the_host(aligners):
    """min(max_len, the largest window + W of the table): 948 columns for the 111-mer under the default scheme (W 277, SPAN
    393, window 671), the read's length below that, and max_len under a scheme the packed kernels refuse."""
    import porechop_amd
    assert aligners("default").middle_paths_cols(4_000_000) == 948 and aligners("default").middle_paths_cols(500) == 500
    assert aligners("refused").middle_paths_cols(70_000) == 70_000
    al = porechop_amd.Aligner(["AATGTACTTCGTTCAGTTACGTATTGCT"])
    try:
        assert al.middle_paths_cols(4_000_000) == 244               # W 70, SPAN 103, window 174
    finally:
        al.close()


def test_a_too_small_pitch_is_refused_before_anything_is_launched(cases, aligners):
    import torch
    al = aligners("default")
    inputs = device_inputs(cases, cases.hits("default")[:64])
    need = (948 + 111 + 15) // 16
    recs = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
    heads = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    ops = torch.zeros((64, need), dtype=torch.int32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    order = ("arena", "read_off", "read_len", "adapter_idx", "read_end", "mask_base", "mask_count", "intervals")

    def call(pitch, n=64):
        return al.lib.pc_middle_paths(al._ctx, *[inputs[k].data_ptr() for k in order], n, MAX_LEN, recs.data_ptr(), heads.data_ptr(),
                                      ops.data_ptr(), pitch, s)
    assert call(need - 1) == -3 and call(need - 1, n=0) == -3           # PC_ERR_BAD_ARG
    al.sync()
    assert int(recs.abs().sum()) == 0 and int(heads.abs().sum()) == 0 and int(ops.abs().sum()) == 0
    assert call(need) == 0
    al.sync()
    assert int(heads[:, 0].min()) > 0


def test_bad_hits_are_reported_and_write_nothing_in_a_child_process():
    """An adapter index outside the table, a read end outside the read, a negative mask count, a mask run that leaves the
    table and a read above max_len: each is checked before the lane touches memory; that hit's outputs stay untouched, the
    others are written, and pc_sync reports the error (tests/middle_paths_child.py)."""
    res = subprocess.run([sys.executable, "-m", "tests.middle_paths_child"], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert res.returncode == 0 and "MIDDLE_PATHS_BAD_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---- through the pipeline and the runner -----------------------------------------------------------------------------------------
def test_phase_c_routes_give_the_same_paths(oracle):
    """phase_c on its three routes (default floor, prove, prefilter) over 2 000 short reads with planted chimeras: the same
    hits, hence the same middle_hit_paths output -- whose records carry every hit's read_start, read_end and identity (the
    call itself raises otherwise) -- and, for every hit, the path align_pairs_paths finds over the masked whole read."""
    import torch
    from porechop_amd.batch import decode_paths
    from porechop_amd.pipeline import AdapterSet, Pipeline, ScanParams
    from porechop_amd.synth import reads_from_strings
    from tests import floorgen
    from tests.golden_io import load_panel
    from tests.test_gpu_pass2_floor import chimeric_reads

    sets = [AdapterSet(a["name"], tuple(a["start"]) if a["start"] else None, tuple(a["end"]) if a["end"] else None) for a in load_panel()]
    pl = Pipeline(sets, ScanParams())
    try:
        matching = [i for i, s in enumerate(pl.sets) if s.name in floorgen.SETS]
        raw = chimeric_reads(random.Random(2000), 2000)
        dreads, norm = reads_from_strings(raw)
        zero = torch.zeros(len(raw), dtype=torch.int32, device="cuda")
        outs = []
        for kw in ({}, {"prove": True}, {"prefilter": True}):
            hits = pl.phase_c(dreads, zero, zero, matching, **kw)
            recs, heads, ops = pl.middle_hit_paths(dreads, zero, zero, hits)
            pl.aligner.sync()
            outs.append((hits, recs.cpu().numpy(), heads.cpu().numpy(), ops.cpu().numpy()))
        hits, recs, heads, ops = outs[0]
        H = int(hits.read.numel())
        assert H >= 250 and hits.rounds >= 3
        for other in outs[1:]:
            for f in ("read", "adapter", "start", "end", "identity"):
                assert torch.equal(getattr(hits, f), getattr(other[0], f)), f
            assert np.array_equal(recs, other[1]) and np.array_equal(heads, other[2]) and np.array_equal(ops, other[3])
        # the masked reads, rebuilt on the host in discovery order
        state, pairs = {}, []
        table = [pl.seq_index[a[1]] for a in pl.middle_adapters]
        for r, a, s, e in zip(hits.read.tolist(), hits.adapter.tolist(), hits.start.tolist(), hits.end.tolist()):
            seq = state.get(r, norm[r])
            seq = seq.decode() if isinstance(seq, bytes) else seq
            pairs.append((seq, table[a]))
            state[r] = seq[:s] + "-" * (e - s) + seq[e:]
        want_recs, want_heads, want_strings = pl.aligner.align_pairs_paths(pairs)
        assert np.array_equal(recs, want_recs) and np.array_equal(heads, want_heads)
        assert decode_paths(heads, ops) == want_strings
    finally:
        pl.close()


def chimeric_fastq(path, seed, n):
    """n ligation reads of 400..1 500 bases as a FASTQ file: most start with the Y adapter's top strand, half end with its
    bottom strand, 8 % hold one or two junctions (bottom + top) in their middle."""
    from tests.pairgen import mutate
    from tests.readgen import Y_BOTTOM, Y_TOP
    rng = random.Random(seed)
    with open(path, "w") as fh:
        for i in range(n):
            seq = "".join(rng.choice("ACGT") for _ in range(rng.randint(400, 1500)))
            if rng.random() < 0.08:
                for _ in range(rng.choice([1, 1, 2])):
                    pos = rng.randint(160, len(seq) - 160)
                    seq = seq[:pos] + mutate(rng, Y_BOTTOM, 0.04) + mutate(rng, Y_TOP, 0.04) + seq[pos:]
            if rng.random() < 0.9:
                seq = mutate(rng, Y_TOP, 0.1)[rng.randint(0, 8):] + seq
            if rng.random() < 0.5:
                e = mutate(rng, Y_BOTTOM, 0.1)
                seq += e[:len(e) - rng.randint(0, 8)]
            fh.write("@lig%05d\n%s\n+\n%s\n" % (i, seq, "5" * len(seq)))
    return str(path)


def test_report_with_middle_paths(tmp_path):
    from porechop_amd import runner
    from porechop_amd.batch import expand_cigar
    from porechop_amd.io import ReadSet
    from porechop_amd.panel import load_panel
    from tests import readgen, ref_pipeline
    inp = chimeric_fastq(tmp_path / "chimeric.fastq", 77, 3000)
    opts = runner.Options()

    def go(tag, streamed=None, **kw):
        out = str(tmp_path / (tag + ".fastq"))
        report = str(tmp_path / (tag + ".tsv"))
        if streamed:
            assert runner.run_streamed(inp, out, None, opts, block_bytes=streamed, report=report, **kw) is not None, "not streamed"
        else:
            runner.run(inp, output=out, options=opts, report=report, **kw)
        with open(report) as f:
            return f.read(), list(readgen.output_md5s(out).values())

    plain, md5_plain = go("plain")
    text, md5 = go("middle", report_middle_paths=True)
    streamed, md5_s = go("streamed", streamed=300_000, report_middle_paths=True)
    both, md5_b = go("both", report_paths=True, report_middle_paths=True)
    # no output byte and none of the 17 columns changes; a streamed run writes the same report
    assert md5 == md5_plain == md5_s == md5_b and streamed == text
    a, b = plain.split("\n"), text.split("\n")
    assert len(a) == len(b) == 3002 and a[-1] == b[-1] == ""
    assert b[0] == a[0] + "\tmiddle_cigars" and len(a[0].split("\t")) == 17
    # with both options the new column comes last, behind the end alignments' two
    rows_both = both.split("\n")
    assert len(rows_both) == len(b) and rows_both[0] == a[0] + "\tstart_cigars\tend_cigars\tmiddle_cigars"
    for row_a, row_b, row_m in zip(a[1:-1], rows_both[1:-1], b[1:-1]):
        cols = row_b.split("\t")
        assert len(cols) == 20 and "\t".join(cols[:17]) == row_a and cols[19] == row_m.split("\t")[17]
    known = {side[0]: side[1] for s in load_panel() for side in (s.start, s.end) if side is not None}
    rs = ReadSet(inp)
    entries, later_rounds = 0, 0
    try:
        for r, (row_a, row_b) in enumerate(zip(a[1:-1], b[1:-1])):
            cols = row_b.split("\t")
            assert len(cols) == 18 and "\t".join(cols[:17]) == row_a, r
            mids = [] if cols[6] == "." else cols[6].split(";")
            cgs = [] if cols[17] == "." else cols[17].split(";")
            assert len(mids) == len(cgs), r
            if not mids:
                continue
            seq = rs.seq(r)
            seq = seq.decode() if isinstance(seq, bytes) else seq
            masked = ref_pipeline.trimmed(seq, int(cols[2]), int(cols[3]))
            for k, (mid, cg) in enumerate(zip(mids, cgs)):
                name, r_start, r_end, identity = mid.rsplit("|", 3)
                read_first, adapter_first, text_ = cg.split("|")
                ops = expand_cigar(text_)
                # The path, laid over the MASKED trimmed read from (read_first, adapter_first), must be the hit: every = / X is
                # checked against the bases on the way, and alignment.cpp's rule over the two gapped rows (pathcheck: from the
                # first to the last column by which both rows have shown a base) gives the entry's read_start and read_end --
                # the path spans exactly read_end - read_start read bases by that count -- and its identity.
                rs_, re_, _, _, _, _, fm, fl = pathcheck.digest_from_path(masked, known[name], int(read_first), int(adapter_first), ops)
                assert (rs_, re_ + 1) == (int(r_start), int(r_end)) and "%.6f" % ((100.0 * fm) / fl) == identity, (r, k, mid, cg)
                assert int(read_first) <= int(r_start) and int(read_first) + sum(op != "D" for op in ops) in (int(r_end), int(r_end) - 1)
                masked = masked[:int(r_start)] + "-" * (int(r_end) - int(r_start)) + masked[int(r_end):]
                entries += 1
                later_rounds += k > 0
    finally:
        rs.close()
    assert entries >= 300 and later_rounds >= 100
