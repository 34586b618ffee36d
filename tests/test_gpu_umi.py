"""UMI extraction on the MI355X (pc_umi_extract / Aligner.umis and what is built on it): the read columns under an adapter's
degenerate rows, taken from the alignment's path on the device.  Everything is compared with tests/umi_ref.py over
tests/wild_ref.py's independent paths; the records also with Aligner.scan_device."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import umi_ref, umigen
from tests.umigen import END_SIZE, PLACEMENTS, SCHEMES, UMI28, UMI67

pytestmark = pytest.mark.gpu

BAD_ARG = -3
RULE = (END_SIZE, 4, 2, 75.0)
FILLER128 = "".join(random.Random(128).choice("ACGT") for _ in range(128))       # 128 rows, no span


def cuda(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


class Case:
    """Windows against one adapter: the arena, and the reference's records and paths per scheme, computed once."""

    def __init__(self, ad, windows, alignments=None):
        self.ad, self.windows = ad, windows
        self.span = umi_ref.span(ad)
        self.arena, self.off, self.len = umigen.lay_out(windows, alignments)
        self._ref = {}

    def ref(self, scheme="default"):
        if scheme not in self._ref:
            from tests import wild_ref
            self._ref[scheme] = wild_ref.align_many([(w, self.ad) for w in self.windows], SCHEMES[scheme], wildcards=True)
        return self._ref[scheme]

    def want(self, scheme="default", side=0, rule=None, count=None):
        recs, paths = self.ref(scheme)
        count = len(self.windows) if count is None else count
        umi = np.array([umi_ref.classify(recs[k], paths[k], self.span, side, rule) for k in range(count)], dtype=np.int32).reshape(count, 4)
        return recs[:count], umi

    def device(self):
        if not hasattr(self, "_dev"):
            self._dev = (cuda(np.frombuffer(self.arena, dtype=np.uint8)), cuda(self.off), cuda(self.len))
        return self._dev


def run(al, case, index, side=0, rule=None, count=None, max_len=END_SIZE):
    arena, off, length = case.device()
    count = len(case.windows) if count is None else count
    recs, umi = al.umis(arena, off[:count].contiguous(), length[:count].contiguous(), index, side, rule=rule, max_len=max_len)
    al.sync()
    assert tuple(recs.shape) == (count, 8) and tuple(umi.shape) == (count, 4)
    return recs.cpu().numpy(), umi.cpu().numpy()


def same_as_scan(al, case, index, recs, count=None):
    """The kernel's records are pc_scan_device's.  (Not for an EMPTY window: there the scans' record is not an alignment's
    -- the packed kernels leave (0, -1, m, 0, ...) --, and pc_umi_extract writes the reference's failure record, field 0 = -1,
    as pc_align_paths and pc_align_batch_host do; the comparison with the reference above covers those windows.)"""
    count = len(case.windows) if count is None else count
    filled = case.len[:count] > 0
    return np.array_equal(recs[filled], scan_records(al, case, index, count)[filled])


def scan_records(al, case, index, count=None):
    import torch
    arena, off, length = case.device()
    count = len(case.windows) if count is None else count
    out = torch.zeros((count, 8), dtype=torch.int32, device="cuda")
    if count:
        al.scan_device(arena, off[:count].contiguous(), length[:count].contiguous(), [index], [0, count], END_SIZE, out)
        al.sync()
    return out.cpu().numpy()


def check(case, got, want, what):
    for name, g, w in (("records", got[0], want[0]), ("umi", got[1], want[1])):
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, (what, name, bad[:5].tolist(), [case.windows[k] for k in bad[:2]], case.ad, g[bad[:3]].tolist(), w[bad[:3]].tolist())


# ---- adapter rows, span placements, window lengths, byte alignments; first in the table and behind 128 rows --------------
@pytest.mark.parametrize("m", [1, 16, 28, 48, 112, 128])
def test_adapter_rows_and_span_placements(m):
    import porechop_amd
    rng = random.Random(1000 + m)
    ads = [umigen.adapter(rng, m, p) for p in PLACEMENTS]
    cases = []
    for ad in ads:
        windows, alignments = [], []
        for n in (0, 1, max(0, m - 1), m, min(END_SIZE, m + 1), 149, 150):
            for a in range(4):
                windows.append(umigen.window(rng, ad, n, umigen.HOWS[(n + a) % 4]))
                alignments.append(a)
        for k in range(8):
            windows.append(umigen.window(rng, ad, rng.randint(1, END_SIZE), umigen.HOWS[k % len(umigen.HOWS)]))
            alignments.append(k)
        cases.append(Case(ad, windows, alignments))
    statuses = set()
    for table, base in ((ads, 0), ([FILLER128] + ads, 1)):
        al = porechop_amd.Aligner(table, SCHEMES["default"], wildcards=True)
        try:
            for k, case in enumerate(cases):
                assert al.umi_span(base + k) == case.span
                got = run(al, case, base + k)
                check(case, got, case.want(), (m, PLACEMENTS[k], base))
                assert same_as_scan(al, case, base + k, got[0]), (m, PLACEMENTS[k], base)
                statuses |= set(got[1][:, 0].tolist())
            if base:
                assert al.umi_span(0) is None
        finally:
            al.close()
    assert {0, 1} <= statuses and (m == 1 or 3 in statuses), statuses


# ---- one adapter, a thousand windows: counts, slicing, schemes, rule and side ---------------------------------------------
@pytest.fixture(scope="module")
def thousand():
    return Case(UMI28, umigen.many_windows(28, UMI28, 1000))


@pytest.fixture(scope="module")
def aligners():
    import porechop_amd
    made = {}

    def get(scheme):
        if scheme not in made:
            made[scheme] = porechop_amd.Aligner([FILLER128[:40], UMI28, UMI67], SCHEMES[scheme], wildcards=True)
        return made[scheme]
    yield get
    for al in made.values():
        al.close()


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_counts(thousand, aligners, count):
    al = aligners("default")
    got = run(al, thousand, 1, count=count)
    check(thousand, got, thousand.want(count=count), count)
    assert same_as_scan(al, thousand, 1, got[0], count)
    if count == 1000:
        span = thousand.span[1] - thousand.span[0] + 1
        ok = got[1][got[1][:, 0] == 0]
        assert set(got[1][:, 0].tolist()) == {0, 1, 3}
        assert (ok[:, 2] == span).any() and (ok[:, 2] > span).any() and (ok[:, 2] < span).any() and (got[1][got[1][:, 0] == 3][:, 2] == 0).any()


def test_slices_give_what_one_launch_gives(thousand, aligners, monkeypatch):
    al = aligners("default")
    whole = run(al, thousand, 1)
    # the budget rule of pc_align_paths over THIS adapter: trace (150 columns x 4 row groups) and operations per lane
    per_pair = END_SIZE * ((len(UMI28) + 7) // 8) * 4 + ((END_SIZE + len(UMI28) + 15) // 16) * 4
    launch = max(64, ((1 << 20) // per_pair) // 64 * 64)
    assert -(-1000 // launch) >= 3
    monkeypatch.setenv("PC_PATHS_SCRATCH_MB", "1")
    sliced = run(al, thousand, 1)
    assert np.array_equal(whole[0], sliced[0]) and np.array_equal(whole[1], sliced[1])
    check(thousand, sliced, thousand.want(), "sliced")


@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_schemes(thousand, aligners, scheme):
    import porechop_amd
    assert porechop_amd.load_library().pc_scores_supported(*SCHEMES[scheme], 28) == (0 if scheme == "refused" else 1)
    al = aligners(scheme)
    got = run(al, thousand, 1, count=210)
    check(thousand, got, thousand.want(scheme, count=210), scheme)
    assert same_as_scan(al, thousand, 1, got[0], 210)
    long_case = Case(UMI67, umigen.many_windows(67, UMI67, 70))
    check(long_case, run(al, long_case, 2), long_case.want(scheme), (scheme, 67))


def test_rule_and_side(thousand, aligners):
    al = aligners("default")
    free = run(al, thousand, 1)
    recs = thousand.ref()[0]
    rs, re_ = recs[:, 0], recs[:, 1] + 1
    ident = np.array([umi_ref.identity(int(r[5]), int(r[6])) if r[0] >= 0 else 0.0 for r in recs])
    ok, high, long_enough = rs >= 0, ident > RULE[3], re_ - rs >= RULE[1]
    # pairs that fail exactly one of the four conditions, so that each of them decides
    assert (ok & ~high & long_enough).any() and (ok & high & ~long_enough).any()
    assert (ok & high & long_enough & (re_ == END_SIZE)).any() and (ok & high & long_enough & (rs == 0)).any()
    for side in (0, 1):
        got = run(al, thousand, 1, side=side, rule=RULE)
        check(thousand, got, thousand.want(side=side, rule=RULE), ("rule", side))
        assert np.array_equal(got[0], free[0])
        flush = (re_ == END_SIZE) if side == 0 else (rs == 0)
        assert (got[1][ok & high & long_enough & flush][:, 0] == 2).all()
        assert (got[1][ok & high & long_enough & ~flush][:, 0] != 2).all()
        assert (got[1][got[1][:, 0] == 2][:, 1:] == np.array([-1, 0, 0])).all() and (got[1][got[1][:, 0] == 1][:, 1:] == np.array([-1, 0, 0])).all()
        # with rule=None the same pairs are extracted
        assert (free[1][got[1][:, 0] == 2][:, 0] != 2).all()


# ---- refusals and the errors the kernel reports ---------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(thousand):
    import porechop_amd
    import torch
    long_umi = FILLER128 + "NN"
    al = porechop_amd.Aligner([FILLER128[:40], UMI28, long_umi], SCHEMES["default"], wildcards=True)
    try:
        arena, off, length = thousand.device()
        recs = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
        umi = torch.zeros((64, 4), dtype=torch.int32, device="cuda")

        def call(index, side=0, n=64):
            return al.lib.pc_umi_extract(al._ctx, arena.data_ptr(), off.data_ptr(), length.data_ptr(), n, END_SIZE, index, side, None,
                                         recs.data_ptr(), umi.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

        def still_works():
            al.sync()
            assert int(recs.abs().sum()) == 0 and int(umi.abs().sum()) == 0         # nothing was launched
            check(thousand, run(al, thousand, 1, count=65), thousand.want(count=65), "after a refusal")

        for index in (-1, 3, 1 << 20):                 # outside the table
            assert call(index) == BAD_ARG
            still_works()
        assert al.umi_span(2) == (128, 129) and call(2) == BAD_ARG           # above 128 rows
        still_works()
        assert al.umi_span(0) is None and call(0) == BAD_ARG                 # no span
        still_works()
        for side in (-1, 2):
            assert call(1, side=side) == BAD_ARG
            still_works()
        assert call(1, n=-1) == BAD_ARG
        still_works()
        assert call(1, n=0) == 0                                             # a no-op
        still_works()
        al.set_wildcards(False)
        assert al.umi_span(1) is None and call(1) == BAD_ARG                 # wildcards off
        with pytest.raises(RuntimeError):
            al.umis(arena, off[:4].contiguous(), length[:4].contiguous(), 1, 0, max_len=END_SIZE)
        al.set_wildcards(True)
        still_works()
        with pytest.raises(RuntimeError):
            al.umi_span(3)
    finally:
        al.close()


def test_a_window_above_max_len_is_reported_and_writes_nothing(thousand, aligners):
    al = aligners("default")
    long_ones = np.nonzero(thousand.len[:64] > 100)[0]
    assert long_ones.size > 0 and (thousand.len[:64] <= 100).any()
    arena, off, length = thousand.device()
    recs, umi = al.umis(arena, off[:64].contiguous(), length[:64].contiguous(), 1, 0, max_len=100)
    with pytest.raises(RuntimeError):
        al.sync()
    recs, umi = recs.cpu().numpy(), umi.cpu().numpy()
    want = thousand.want(count=64)
    short = thousand.len[:64] <= 100
    assert not recs[~short].any() and not umi[~short].any()
    assert np.array_equal(recs[short], want[0][short]) and np.array_equal(umi[short], want[1][short])
    check(thousand, run(al, thousand, 1, count=64), want, "after the report")


# ---- windows behind byte 2^32 of the arena ----------------------------------------------------------------------------------
def test_far_offsets(thousand, aligners):
    import torch
    from tests import fargen
    free, _ = torch.cuda.mem_get_info()
    if free < (12 << 30):
        pytest.skip("less than 12 GB of device memory free (%.1f GB)" % (free / 2**30))
    al = aligners("default")
    count = 130
    block = thousand.arena[:int(thousand.off[count - 1] + thousand.len[count - 1])]
    arena = torch.empty(fargen.ARENA_BYTES, dtype=torch.uint8, device="cuda")
    try:
        # one copy starts behind 2^32 at an odd byte; another lies across 2^32, which falls inside its 40th window
        starts = [fargen.BEYOND32_START, fargen.B32 - int(thousand.off[40]) - 7]
        assert thousand.len[40] > 7 and starts[1] + len(block) < starts[0]
        offs = []
        for s in starts:
            arena[s:s + len(block)] = cuda(np.frombuffer(block, dtype=np.uint8))
            offs.append(thousand.off[:count] + s)
        off = cuda(np.concatenate(offs))
        length = cuda(np.concatenate([thousand.len[:count]] * 2))
        recs, umi = al.umis(arena, off, length, 1, 1, rule=RULE, max_len=END_SIZE)
        al.sync()
        want = thousand.want(side=1, rule=RULE, count=count)
        for k in range(2):
            check(thousand, (recs.cpu().numpy()[k * count:(k + 1) * count], umi.cpu().numpy()[k * count:(k + 1) * count]), want, ("far", k))
    finally:
        del arena
        torch.cuda.empty_cache()


# ---- Pipeline.end_umis: which adapter's UMI a read keeps ---------------------------------------------------------------------
A_START = "ACGTACGTAC" + "NNNNNNNN" + "GGATCCGGAT"       # set A: any base under the span
B_START = "ACGTACGTAC" + "VVVVVVVV" + "GGATCCGGAT"       # set B: the same flanks, A/C/G under the span
A_END = "GCTAGTCAGGTC" + "NNNNNNNN" + "CTGATCCATGAGTC"


def _end_umi_reads():
    """2 000 reads: a copy of the start adapters with a UMI of A/C/G (both sets align it with the same score: a tie), one with
    T's in the UMI (set A scores higher), the end adapter alone, both ends, neither; every seventh read longer than a window."""
    rng = random.Random(2000)
    reads = []
    for k in range(2000):
        kind = k % 5
        body = umigen.noise(rng, 200 if k % 7 == 3 else rng.randint(20, 80))
        start = end = ""
        if kind in (0, 3):
            start = "ACGTACGTAC" + umigen.noise(rng, 8, "ACG") + "GGATCCGGAT"
        if kind == 1:
            start = "ACGTACGTAC" + "T" + umigen.noise(rng, 6, "ACGT") + "T" + "GGATCCGGAT"
        if kind in (2, 3):
            end = umigen.instance(rng, A_END)
        reads.append(start + body + end)
    return reads


def _choose(refs, order, first_shift):
    """The rule of Pipeline.end_umis over the reference's results: status 0, the highest score, ties to the first in order."""
    R = refs[order[0]][0].shape[0]
    best = np.full((R, 4), -1, dtype=np.int64)
    best[:, 2:] = 0
    score = np.zeros(R, dtype=np.int64)
    by_score = by_order = 0
    for rank, si in enumerate(order):
        recs, umi = refs[si]
        for r in range(R):
            if umi[r, 0] != 0:
                continue
            if best[r, 0] < 0 or recs[r, 4] > score[r]:
                by_score += best[r, 0] >= 0
                best[r] = (si, umi[r, 1] + first_shift[r] if umi[r, 1] >= 0 else -1, umi[r, 2], umi[r, 3])
                score[r] = recs[r, 4]
            elif recs[r, 4] == score[r]:
                by_order += 1
    return best, by_score, by_order


def test_pipeline_end_umis_score_rule_and_tie_rule():
    import torch
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import AdapterSet, DeviceReads, Pipeline, ScanParams
    reads = _end_umi_reads()
    builtin = load_panel()
    sets = builtin + [AdapterSet("kit A", ("A_start", A_START), ("A_end", A_END)), AdapterSet("kit B", ("B_start", B_START), None)]
    ia, ib = len(builtin), len(builtin) + 1
    arena = "".join(reads).encode() + b"N" * 64
    length = np.array([len(r) for r in reads], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(length[:-1].astype(np.int64))]).astype(np.int64)
    starts = [r[:END_SIZE] for r in reads]
    ends = [r[-END_SIZE:] for r in reads]
    shift = np.maximum(length.astype(np.int64) - END_SIZE, 0)
    ref_start = {ia: umi_ref.umi_many(starts, A_START, SCHEMES["default"], 0, RULE), ib: umi_ref.umi_many(starts, B_START, SCHEMES["default"], 0, RULE)}
    ref_end = {ia: umi_ref.umi_many(ends, A_END, SCHEMES["default"], 1, RULE)}
    pl = Pipeline(sets, ScanParams(wildcards=True))
    try:
        dev_reads = DeviceReads(cuda(np.frombuffer(arena, dtype=np.uint8)), cuda(off), cuda(length))
        assert [(a[0], a[1]) for a in pl.umi_adapters(range(len(sets)))] == [(0, ia), (1, ia), (0, ib)]
        decided = {}
        for order in ([ia, ib], [ib, ia]):
            got = pl.end_umis(dev_reads, order)
            pl.aligner.sync()
            want_start, by_score, by_order = _choose(ref_start, order, np.zeros(len(reads), dtype=np.int64))
            want_end, _, _ = _choose(ref_end, [ia], shift)
            decided[tuple(order)] = (by_score, by_order)
            for side, want in ((0, want_start), (1, want_end)):
                have = torch.stack([x.to(torch.int64) for x in got[side]], dim=1).cpu().numpy()
                bad = np.nonzero((have != want).any(axis=1))[0]
                assert bad.size == 0, (order, side, bad[:5].tolist(), have[bad[:3]].tolist(), want[bad[:3]].tolist())
            # the ties went to whichever set came first, the reads with a T under the span to set A either way
            start_set = got[0][0].cpu().numpy()
            assert (start_set[0::5] == order[0]).all() and (start_set[1::5] == ia).all() and (start_set[4::5] == -1).sum() > 200
            assert (got[1][0].cpu().numpy()[2::5] == ia).all()
        # both rules decided: with B first, A takes a read from it by score; with A first, B's equal score loses by order
        assert decided[(ib, ia)][0] >= 300 and decided[(ia, ib)][1] >= 300, decided
        assert pl.stats["umi_pairs"] == 2 * 3 * len(reads)
        # the UMI's bases, from the coordinates: a read of kind 0 carries its eight bases at 10 .. 17
        first, n = got[0][1].cpu().numpy(), got[0][2].cpu().numpy()
        assert first[0] == 10 and n[0] == 8 and reads[0][10:18] == starts[0][first[0]:first[0] + n[0]]
        # the end side in whole-read coordinates: a read longer than a window that carries the end adapter
        k = next(k for k in range(2000) if k % 5 == 2 and len(reads[k]) > END_SIZE)
        assert got[1][1].cpu().numpy()[k] == len(reads[k]) - len(A_END) + 12 and got[1][2].cpu().numpy()[k] == 8
    finally:
        pl.close()


# ---- the runner on the library: the bytes the CPU test states ----------------------------------------------------------------
def test_runner_writes_the_stated_files(tmp_path):
    from porechop_amd import runner
    from tests import umi_runner_case
    reads, out_records, rows = umi_runner_case.build()
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(reads))
    opts = runner.Options()
    opts.check_reads = 3
    for tag, streamed in (("whole", None), ("streamed", 4000)):
        out, report = tmp_path / ("out_%s.fastq" % tag), tmp_path / ("umis_%s.tsv" % tag)
        kw = dict(adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, umi=True, umi_report=str(report))
        if streamed:
            res = runner.run_streamed(str(inp), str(out), None, opts, block_bytes=streamed, **kw)
            assert res is not None, "not streamed"
        else:
            res = runner.run(str(inp), output=str(out), options=opts, **kw)
        assert out.read_text() == umi_runner_case.fastq_text(out_records), tag
        assert report.read_text() == umi_runner_case.report_text(rows), tag
        assert len(res.umis) == 12 and res.umis[7] == (None, None)


def test_without_umi_a_wildcard_run_is_what_it_was(tmp_path):
    """runner.run(wildcards=True) without the option: the pieces the wildcard runner test states (tests/wild_runner_case.py:
    40 reads trimmed by 30 and 24 bases, a chimera split in two), under the input's own headers; umi=False is that run."""
    from porechop_amd import runner
    from tests import wild_runner_case
    reads, expected = wild_runner_case.build()
    inp = wild_runner_case.write_fastq(tmp_path / "reads.fastq", reads)
    pieces = [p for per_read in expected for p in per_read]
    names = ["read_%d" % (k + 1) for k in range(40)] + ["read_41_1", "read_41_2"]
    want = "".join("@%s\n%s\n+\n%s\n" % (n, s, "5" * len(s)) for n, s in zip(names, pieces))
    for tag, kw in (("plain", {}), ("off", dict(umi=False, umi_report=None))):
        out = tmp_path / ("out_%s.fastq" % tag)
        res = runner.run(inp, output=str(out), adapter_panel=wild_runner_case.adapter_sets(), wildcards=True, **kw)
        assert out.read_text() == want, tag
        assert res.umis is None and (res.start_trim == 30).all() and (res.end_trim == 24).all()


def test_command_line_writes_tags_and_report(tmp_path):
    """python -m porechop_amd.custom ... --only_custom --wildcards --umi --umi_report: the stated files once more."""
    from porechop_amd import custom
    from tests import umi_runner_case
    reads, out_records, rows = umi_runner_case.build()
    inp, fa = tmp_path / "reads.fastq", tmp_path / "umi.fasta"
    inp.write_text(umi_runner_case.fastq_text(reads))
    fa.write_text(">%s_start\n%s\n>%s_end\n%s\n" % (umi_runner_case.KIT, umi_runner_case.START, umi_runner_case.KIT, umi_runner_case.END))
    out, report = tmp_path / "out.fastq", tmp_path / "umis.tsv"
    custom.main(["-i", str(inp), "-o", str(out), "--adapters", str(fa), "--only_custom", "--wildcards", "--umi", "--umi_report", str(report),
                 "--check_reads", "3", "-v", "0"])
    assert out.read_text() == umi_runner_case.fastq_text(out_records)
    assert report.read_text() == umi_runner_case.report_text(rows)
