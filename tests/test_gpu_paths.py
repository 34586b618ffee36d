"""Alignment paths on the MI355X (pc_align_paths / Aligner.align_paths and what is built on them).

One seeded list of 300 (window, adapter) pairs -- window lengths {0, 1, 2, 15, 16, 17, 150, 300} and adapter lengths
{1, 7, 8, 9, 16, 17, 28, 33, 128} mixed within every wave, one adapter holding an N, windows at odd byte offsets,
overlapping and repeated windows, the last window ending at the arena's last byte -- runs under four schemes: the
default, a linear one, gap_open > gap_extend, and one the packed kernels refuse.  Every pair of every call is checked:
the records equal align_host's (for the first three schemes: the packed fp16 / int16 kernels) and the oracle's, and the
returned path satisfies tests/pathcheck.py (b)-(g): replayed base by base it stays in the rectangle, ends at the oracle's
end cell, realises the score and reproduces the record through alignment.cpp's rule.
"""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import pathcheck
from tests.pairgen import mutate

pytestmark = pytest.mark.gpu

WINDOW_LENGTHS = (0, 1, 2, 15, 16, 17, 150, 300)
ADAPTER_LENGTHS = (1, 7, 8, 9, 16, 17, 28, 33, 128)
SCHEMES = {"default": (3, -6, -5, -2), "linear": (3, -6, -4, -4), "open_above_extend": (3, -6, -2, -5), "refused": (3, -6, 0, -2)}
NPAIRS = 300
MAX_LEN = 300


class Cases:
    def __init__(self):
        rng = random.Random(417)
        self.adapters = ["".join(rng.choice("ACGT") for _ in range(m)) for m in ADAPTER_LENGTHS]
        self.adapters[4] = self.adapters[4][:5] + "N" + self.adapters[4][6:]
        windows, off, length, idx, pos = [], [], [], [], 0
        for k in range(NPAIRS - 40):
            n = WINDOW_LENGTHS[(k * 5 + k // 8) % 8] if k < NPAIRS - 41 else 150      # (the last one is not empty)
            a = (k * 7 + k // 9) % 9
            body = [rng.choice("ACGTACGTACGTNacgtU-X") for _ in range(n)]
            if rng.random() < 0.7 and n >= 15:
                cp = mutate(rng, self.adapters[a], rng.choice((0.0, 0.05, 0.15, 0.3)))[:n]
                at = rng.randint(0, n - len(cp))
                body[at:at + len(cp)] = cp
            windows.append("".join(body))
            off.append(pos); length.append(n); idx.append(a)
            pos += n
        self.arena = "".join(windows).encode("latin-1")
        assert off[-1] + length[-1] == len(self.arena) and length[-1] > 0       # a window ends at the arena's last byte
        for k in range(40):                                                        # overlapping and repeated windows
            src = (k * 11) % (NPAIRS - 40)
            if k % 2:
                off.append(off[src]); length.append(length[src])                   # the same window, another adapter
            else:
                n = WINDOW_LENGTHS[k % 8]
                at = min(max(0, off[src] - 3), len(self.arena) - n)
                off.append(at); length.append(n)
            idx.append((k * 5 + 2) % 9)
        # interleave them so that every wave holds some
        order = list(range(NPAIRS))
        random.Random(3).shuffle(order)
        self.off = np.array(off, dtype=np.int64)[order]
        self.len = np.array(length, dtype=np.int32)[order]
        self.idx = np.array(idx, dtype=np.int32)[order]
        assert int((self.off % 2).sum()) > 50 and set(self.len.tolist()) == set(WINDOW_LENGTHS) and set(self.idx.tolist()) == set(range(9))
        text = self.arena.decode("latin-1")
        self.reads = [text[o:o + n] for o, n in zip(self.off.tolist(), self.len.tolist())]
        self._want = {}

    def want(self, oracle, name):
        """The oracle's results of all pairs under a scheme, computed once."""
        if name not in self._want:
            self._want[name] = [oracle.align_raw(r, self.adapters[a], SCHEMES[name]) for r, a in zip(self.reads, self.idx.tolist())]
        return self._want[name]

    def device(self):
        import torch
        if not hasattr(self, "_dev"):
            self._dev = tuple(torch.from_numpy(np.array(x)).cuda() for x in (np.frombuffer(self.arena, dtype=np.uint8), self.off, self.len, self.idx))
        return self._dev


@pytest.fixture(scope="module")
def cases():
    return Cases()


@pytest.fixture(scope="module")
def aligners(cases):
    import porechop_amd
    made = {}

    def get(name):
        if name not in made:
            made[name] = porechop_amd.Aligner(cases.adapters, SCHEMES[name])
        return made[name]
    yield get
    for al in made.values():
        al.close()


def run(al, cases, count):
    from porechop_amd.batch import decode_paths
    arena, off, length, idx = cases.device()
    recs, heads, ops = al.align_paths(arena, off[:count].contiguous(), length[:count].contiguous(), idx[:count].contiguous(), max_len=MAX_LEN)
    al.sync()
    assert tuple(recs.shape) == (count, 8) and tuple(heads.shape) == (count, 4) and int(ops.shape[0]) == count
    recs, heads, ops = recs.cpu().numpy(), heads.cpu().numpy(), ops.cpu().numpy()
    return recs, heads, ops, decode_paths(heads, ops)


def check_all(cases, oracle, name, recs, heads, strings):
    want = cases.want(oracle, name)
    for p in range(recs.shape[0]):
        where = (name, p, cases.reads[p], cases.adapters[cases.idx[p]])
        assert recs[p].tolist() == pathcheck.oracle_record(want[p]), where
        try:
            pathcheck.check_path(cases.reads[p], cases.adapters[cases.idx[p]], SCHEMES[name], recs[p], heads[p], strings[p], want[p])
        except AssertionError as e:
            raise AssertionError("%r: %s" % (where, e))


@pytest.mark.parametrize("name", list(SCHEMES))
def test_every_pair_of_every_scheme(cases, aligners, oracle, name):
    al = aligners(name)
    recs, heads, ops, strings = run(al, cases, NPAIRS)
    check_all(cases, oracle, name, recs, heads, strings)
    # exactly the records the scans give for the same pairs
    host = al.align_host(cases.arena, cases.off, cases.len, cases.idx)
    assert np.array_equal(recs, host), np.nonzero((recs != host).any(axis=1))[0][:10]
    # the data exercises something: matches, gapped paths and empty ones occur under every scheme; under the default and
    # the linear one also mismatches (where two gap steps cost less than a mismatch, as under the other two, no optimal
    # path holds an X), and under the default one both kinds of gap
    joined = "".join(strings)
    assert "=" in joined and ("I" in joined or "D" in joined)
    assert name not in ("default", "linear") or "X" in joined
    assert name != "default" or ("I" in joined and "D" in joined)
    assert any(h[0] == 0 and n > 0 for h, n in zip(heads, cases.len))


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 200])
def test_pair_counts(cases, aligners, oracle, count):
    recs, heads, ops, strings = run(aligners("default"), cases, count)
    check_all(cases, oracle, "default", recs, heads, strings)


def test_slices_give_what_one_launch_gives(cases, aligners, oracle, monkeypatch):
    al = aligners("default")
    whole = run(al, cases, NPAIRS)
    # the documented budget rule: a launch holds floor(budget / (max_len * row groups of the longest adapter * 4 bytes)) pairs,
    # rounded down to a multiple of 64, but never fewer than 64
    per_pair = MAX_LEN * ((max(ADAPTER_LENGTHS) + 7) // 8) * 4
    launch = max(64, ((1 << 20) // per_pair) // 64 * 64)
    assert -(-NPAIRS // launch) >= 3
    monkeypatch.setenv("PC_PATHS_SCRATCH_MB", "1")
    sliced = run(al, cases, NPAIRS)
    for a, b in zip(whole[:3], sliced[:3]):
        assert np.array_equal(a, b)
    check_all(cases, oracle, "default", sliced[0], sliced[1], sliced[3])


def test_pitch_bound_and_the_longest_path(oracle):
    """ops_pitch_words one below ceil((max_len + longest adapter) / 16) is PC_ERR_BAD_ARG; at the bound the longest path
    there is fits.  A path ends where it first reaches row 0 or column 0, so over n x m cells it has at most n + m - 1
    steps (from (1, 1) a gap step already lands on the border: only a diagonal step reaches (0, 0)) -- n + m is not
    attainable.  All-A against all-C, 16 bases each, under (1, -100, 5, -1), where opening a gap is rewarded, walks up the
    last column and along row 1: 31 steps, the second of the two dwords in use.  (Under a scheme whose gaps cost nothing
    the scout never leaves (m, 0) and the path is empty.)  The oracle confirms the 31 before the GPU is asked."""
    import torch
    import porechop_amd
    from porechop_amd.batch import decode_paths
    scores, rd, ad = (1, -100, 5, -1), "A" * 16, "C" * 16
    want = oracle.align_raw(rd, ad, scores)
    assert (want.end_i, want.end_j) == (16, 16)
    assert want.path_len - want.read_start - want.adapter_start == 31 == len(rd) + len(ad) - 1
    assert oracle.align_raw(rd, ad, (1, -1, 0, 0)).end_j == 0
    al = porechop_amd.Aligner([ad], scores)
    try:
        arena = torch.from_numpy(np.frombuffer(rd.encode(), dtype=np.uint8).copy()).cuda()
        off = torch.zeros(1, dtype=torch.int64, device="cuda")
        length = torch.full((1,), 16, dtype=torch.int32, device="cuda")
        idx = torch.zeros(1, dtype=torch.int32, device="cuda")
        recs = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
        heads = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        ops = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(pitch, n=1):
            return al.lib.pc_align_paths(al._ctx, arena.data_ptr(), off.data_ptr(), length.data_ptr(), idx.data_ptr(), n, 16,
                                         recs.data_ptr(), heads.data_ptr(), ops.data_ptr(), pitch, s)
        assert call(1) == -3 and call(1, n=0) == -3                     # PC_ERR_BAD_ARG, before anything is launched
        al.sync()
        assert int(heads.abs().sum()) == 0 and int(recs.abs().sum()) == 0
        assert call(2) == 0
        al.sync()
        h = heads.cpu().numpy()
        assert h[0].tolist()[:3] == [31, 1, 0]
        strings = decode_paths(h, ops.cpu().numpy())
        assert strings[0].count("I") + strings[0].count("D") == 31
        pathcheck.check_path(rd, ad, scores, recs.cpu().numpy()[0], h[0], strings[0], want)
    finally:
        al.close()


def test_host_convenience_and_the_c_formatter(cases, aligners, oracle):
    from porechop_amd.batch import cigar, expand_cigar
    al = aligners("default")
    pairs = [(cases.reads[p], int(cases.idx[p])) for p in range(40)]
    recs, heads, strings = al.align_pairs_paths(pairs)
    check_all(cases, oracle, "default", recs, heads, strings)
    assert np.array_equal(recs, al.align_pairs(pairs))
    with pytest.raises(ValueError):
        al.align_pairs_paths([("ACGT", len(cases.adapters))])
    # pc_path_cigar over the words as the device wrote them
    _, h, ops, full = run(al, cases, 40)
    for p in range(40):
        words = np.ascontiguousarray(ops[p]).view(np.uint32)
        need = al.lib.pc_path_cigar(words.ctypes.data, int(h[p][0]), None, 0)
        buf = ctypes.create_string_buffer(need + 1)
        assert al.lib.pc_path_cigar(words.ctypes.data, int(h[p][0]), buf, need + 1) == need
        assert buf.value.decode() == cigar(full[p]) and expand_cigar(buf.value.decode()) == full[p]


def test_a_bad_pair_is_reported_and_writes_nothing(cases, aligners):
    """An adapter index outside the table and a window above max_len: the kernel leaves the pair's outputs alone, the others
    get theirs, and pc_sync reports PC_ERR_INTERNAL (the indices live on the device: the call makes no host round trip)."""
    import torch
    al = aligners("default")
    arena, off, length, idx = cases.device()
    good = run(al, cases, 64)
    bad_idx = idx[:64].clone()
    bad_idx[5] = len(cases.adapters)
    bad_idx[6] = -1
    recs, heads, ops = al.align_paths(arena, off[:64].contiguous(), length[:64].contiguous(), bad_idx, max_len=MAX_LEN)
    with pytest.raises(RuntimeError):
        al.sync()
    recs, heads = recs.cpu().numpy(), heads.cpu().numpy()
    keep = np.array([p not in (5, 6) for p in range(64)])
    assert np.array_equal(recs[keep], good[0][keep]) and np.array_equal(heads[keep], good[1][keep])
    assert not recs[~keep].any() and not heads[~keep].any() and not ops.cpu().numpy()[~keep].any()
    long_one = int(np.argmax(cases.len[:64]))
    recs, heads, ops = al.align_paths(arena, off[:64].contiguous(), length[:64].contiguous(), idx[:64].contiguous(),
                                      max_len=int(cases.len[long_one]) - 1)
    with pytest.raises(RuntimeError):
        al.sync()
    assert not recs.cpu().numpy()[long_one].any()
    al.sync()                                                        # (the error word was cleared)


def test_far_offsets(oracle):
    """The block of tests/fargen.py at its four placements in the 4.3 GB arena: the three far placements equal the one at
    byte 0 element for element in records, heads and operations, and that one passes the per-pair checks."""
    import torch
    import porechop_amd
    from porechop_amd.batch import decode_paths
    from tests.fargen import PLACEMENTS
    from tests.test_gpu_far_offsets import NEED_FREE, Far
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip("less than 12 GB of device memory free (%.1f GB)" % (free / 2**30))
    f = Far()
    try:
        f.ensure("mixed")
        al = porechop_amd.Aligner(f.dp, (3, -6, -5, -2))
        idx = np.tile(np.arange(f.n, dtype=np.int32) % len(f.dp), len(PLACEMENTS))
        recs, heads, ops = al.align_paths(f.arena, f.d_off, f.d_len, torch.from_numpy(idx).cuda(), max_len=f.max_len)
        al.sync()
        recs, heads, ops = (f.by_placement(x.cpu().numpy()) for x in (recs, heads, ops))
        al.close()
        for k, name in enumerate(PLACEMENTS[1:], 1):
            for what, x in (("records", recs), ("heads", heads), ("operations", ops)):
                assert np.array_equal(x[k], x[0]), (name, what)
        strings = decode_paths(heads[0], ops[0])
        for p in range(f.n):
            ad = f.dp[idx[p]]
            want = oracle.align_raw(f.block.reads[p], ad, (3, -6, -5, -2))
            assert recs[0][p].tolist() == pathcheck.oracle_record(want), p
            pathcheck.check_path(f.block.reads[p], ad, (3, -6, -5, -2), recs[0][p], heads[0][p], strings[p], want)
    finally:
        f.release()


# ---- the consumers: the explain report and adapter discovery ------------------------------------------------------------------
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_CASES = {"no_barcode_calls": "native_check20", "barcode_bins": "native_bins_two"}


def run_report(name, workdir, tag, streamed_block=None, **kw):
    """One run of a runner case with a report -> (report text, {output file -> md5}, input path)"""
    from porechop_amd import runner
    from tests import readgen
    from tests.runner_cases import load_cases, options_from_argv
    case = load_cases()[name]
    inp = readgen.build_dataset(case["dataset"], os.path.join(workdir, "datasets_" + tag))
    opts = options_from_argv(case["argv"])
    work = os.path.join(workdir, tag)
    os.makedirs(work)
    target = os.path.join(work, "bins" if case["mode"] == "b" else case["mode"][2:])
    out = {"barcode_dir": target} if case["mode"] == "b" else {"output": target}
    report = os.path.join(work, "report.tsv")
    if streamed_block:
        res = runner.run_streamed(inp, out.get("output"), out.get("barcode_dir"), opts, block_bytes=streamed_block, report=report, **kw)
        assert res is not None, "not streamed"
    else:
        runner.run(inp, options=opts, report=report, **out, **kw)
    with open(report) as f:
        return f.read(), readgen.output_md5s(target), inp, opts


def sets_by_name():
    """The panel's adapter sets and the full-sequence barcode sets a run derives from them, by name."""
    from porechop_amd import panel as rules
    panel = rules.load_panel()
    sets = {s.name: s for s in panel}
    for number in range(1, 97):
        for make in (rules.full_native_barcode, rules.full_rapid_barcode_old, rules.full_rapid_barcode_new):
            try:
                s = make(panel, number)
            except StopIteration:
                continue                          # the kit has no barcode of this number
            sets[s.name] = s
    return sets


@pytest.mark.parametrize("which", list(REPORT_CASES))
def test_report_with_paths(tmp_path, which):
    from porechop_amd.batch import expand_cigar
    from porechop_amd.io import ReadSet
    name = REPORT_CASES[which]
    plain, md5_plain, inp, opts = run_report(name, str(tmp_path), "plain")
    text, md5, _, _ = run_report(name, str(tmp_path), "paths", report_paths=True)
    streamed, md5_s, _, _ = run_report(name, str(tmp_path), "streamed", streamed_block=6000, report_paths=True)
    # the option changes no output byte and none of the 17 columns; a streamed run writes the same report
    assert md5 == md5_plain == md5_s and streamed == text
    a, b = plain.split("\n"), text.split("\n")
    assert len(a) == len(b) > 100 and a[-1] == b[-1] == ""
    assert b[0] == a[0] + "\tstart_cigars\tend_cigars" and len(a[0].split("\t")) == 17
    sets = sets_by_name()
    rs = ReadSet(inp)
    entries = 0
    try:
        for r, (row_a, row_b) in enumerate(zip(a[1:-1], b[1:-1])):
            cols = row_b.split("\t")
            assert len(cols) == 19 and "\t".join(cols[:17]) == row_a, r
            seq = rs.seq(r)
            seq = seq.decode() if isinstance(seq, bytes) else seq
            for side, al_col, cg_col in ((0, cols[4], cols[17]), (1, cols[5], cols[18])):
                als = [] if al_col == "." else al_col.split(";")
                cgs = [] if cg_col == "." else cg_col.split(";")
                assert len(als) == len(cgs), (r, side)
                window = seq[:opts.end_size] if side == 0 else seq[-opts.end_size:]
                for al, cg in zip(als, cgs):
                    set_name, full, aligned, r_start, r_end = al.rsplit("|", 4)
                    adapter = (sets[set_name].start if side == 0 else sets[set_name].end)[1]
                    read_first, adapter_first, text_ = cg.split("|")
                    ops = expand_cigar(text_)
                    rs_, re_, _, _, am, al_len, fm, fl = pathcheck.digest_from_path(window, adapter, int(read_first), int(adapter_first), ops)
                    got = "%s|%.6f|%.6f|%d|%d" % (set_name, (100.0 * fm) / fl, (100.0 * am) / al_len, rs_, re_ + 1)
                    assert got == al, (r, side, got, al, cg)
                    entries += 1
    finally:
        rs.close()
    assert entries > 100


def test_report_paths_need_a_report(tmp_path):
    from porechop_amd import runner
    with pytest.raises(runner.UsageError):
        runner.run(str(tmp_path / "none.fastq"), output=str(tmp_path / "out.fastq"), report_paths=True)


def test_discover_alignments_on_the_command_line(tmp_path):
    """discover --alignments on the planted file of tests/test_gpu_discover.py's recipe: under the line of each found sequence
    three lines whose read row and adapter row, with the gaps taken out, are substrings of the found sequence and of its
    nearest known adapter; without the option the output is what it was."""
    from porechop_amd.panel import load_panel
    from tests import kmer_model as km
    from tests.test_gpu_discover import NEW_END, NEW_START, write_fastq
    path = write_fastq(tmp_path / "new.fastq", km.planted_reads(3000, 0.8, 0.08, 7, NEW_START, NEW_END))
    known = {side[0]: side[1] for s in load_panel() for side in (s.start, s.end) if side is not None}

    def cli(*extra):
        res = subprocess.run([sys.executable, "-m", "porechop_amd.discover", "-i", path] + list(extra), cwd=REPO, capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout.split("\n")
    plain, drawn = cli(), cli("--alignments")
    assert plain[-1] == "" and [l for l in drawn if not l.startswith("  ")] == plain
    rows = [l.split("\t") for l in plain[1:-1]]
    assert [r[1] for r in rows] == [NEW_START, NEW_END]
    at = 1
    for r in rows:
        assert drawn[at].split("\t") == r
        top, mid, bottom = (l[2:] for l in drawn[at + 1:at + 4])
        assert all(l.startswith("  ") for l in drawn[at + 1:at + 4]) and len(top) == len(mid) == len(bottom) > 0
        assert top.replace("-", "") in r[1] and bottom.replace("-", "") in known[r[5]]
        assert all((m == "|") == (t == u and t != "-") for t, m, u in zip(top, mid, bottom)) and "|" in mid
        at += 4
    assert drawn[at:] == [""]
