"""Per-base quality values of the UMI consensus on the MI355X (pc_consensus_round_quality / Aligner.consensus_round(qual_table=...),
consensus_call_kernel<true> of csrc/pc_consensus.hip) against the numpy model consensus.round_host(qual_table=...) -- itself
checked against hand-stated pile-ups in tests/test_consensus_quality_cpu.py, and the two margin functions against a naive
restatement in tests/test_consensus_quality_host.py.  Everything must be EQUAL: qualities, consensus bytes, lengths, voters.
Template lengths 1, 2, 254 .. 257 and 600 are the edges of the call kernel's chunks of 256 positions (a template of la bases has
la + 1 positions: 255 is one chunk, 256 is two); the table (7 m + 3) % 94 gives neighbouring margins different values, so
an index off by one shows."""
import ctypes
import random

import numpy as np
import pytest

from porechop_amd import consensus as cs

pytestmark = pytest.mark.gpu

BAD_ARG = -3
TABLE = ((7 * np.arange(256) + 3) % 94).astype(np.uint8)
MARGIN = np.minimum(np.arange(256), 93).astype(np.uint8)       # on the model only: shows the margin itself
LENGTHS = [1, 2, 254, 255, 256, 257, 600]
BANDS = [8, 64]


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    from tests.umigen import SCHEMES
    a = porechop_amd.Aligner(["ACGTACGTACGT"], SCHEMES["default"])
    yield a
    a.close()


def _other(ch, k=1):
    return "ACGT"[("ACGT".index(ch) + k) % 4]


def _members(rng, tmpl):
    """Five members of a template of at least 254 bases with PLANNED edits -- (position, members, edit) -- and 1 % of random
    substitutions on top.  The insertions' drift is taken back by deletions a few columns on, so that every member stays inside
    band 8."""
    t = tmpl.decode()
    la = len(t)
    plan = {}                                                   # position -> {member: (bases put before the column, the column's base or "")}

    def put(pos, who, before="", base=None):
        for m in who:
            plan.setdefault(pos, {})[m] = (before, t[pos] if base is None else base)

    put(10, [0], base=_other(t[10]))                            # 4 : 1 (+ the template)
    put(20, [0, 1], base=_other(t[20]))                         # 3 : 2
    put(30, [0], base=_other(t[30], 1))                         # 3 : 1 : 1
    put(30, [1], base=_other(t[30], 2))
    put(40, [0, 1], base=_other(t[40], 1))                      # 2 : 2 : 1
    put(40, [2, 3], base=_other(t[40], 2))
    put(50, [0, 1, 2], base="N")                                # three abstain
    put(55, [0, 1, 2, 3, 4], base="N")                          # all abstain: the template's vote alone
    put(60, [0], base="")                                       # one deletion
    put(70, [0, 1, 2], base="")                                 # the column is deleted
    put(80, [0, 1, 2, 3], before=_other(t[80], 2) if _other(t[80], 2) != t[79] else _other(t[80], 1))      # one base, four of five
    put(84, [0, 1, 2, 3], base="")
    put(90, [0, 1, 2], before=_other(t[90], 2) if _other(t[90], 2) != t[89] else _other(t[90], 1))         # three of five
    put(94, [0, 1, 2], base="")
    put(100, [0, 1], before="T" if "T" not in (t[99], t[100]) else "A")                                      # the holders disagree
    put(100, [2], before="C" if "C" not in (t[99], t[100]) else "G")
    put(104, [0, 1, 2], base="")
    put(110, [0, 1, 2, 3], before="GA")                         # two bases
    put(113, [0, 1, 2, 3], base="")
    put(116, [0, 1, 2, 3], base="")
    put(130, [0, 1, 2, 3], before="ACGTA")                      # five bases: four have a slot
    for pos in (134, 137, 140, 143, 146):
        put(pos, [0, 1, 2, 3], base="")
    put(160, [4], before="TTTTT")                               # five bases in one member: not emitted
    for pos in (164, 167, 170, 173, 176):
        put(pos, [4], base="")
    for pos in (253, 254, 255, 256):                            # the chunk's edge
        if pos < la:
            put(pos, [pos % 5], base=_other(t[pos]))
    put(la - 1, [1, 2, 3], base=_other(t[la - 1]))              # the last column
    out = []
    for m in range(5):
        s = []
        for pos, ch in enumerate(t):
            before, base = plan.get(pos, {}).get(m, ("", ch))
            if base == ch and rng.random() < 0.01:
                base = _other(ch, rng.randrange(1, 4))
            s.append(before + base)
        if m < 3:
            s.append("G")                                       # an insertion behind the last column: gap la
        out.append("".join(s).encode())
    return out


class Case:
    def __init__(self, tmpls, members, groups):
        self.tmpls, self.members, self.groups = list(tmpls), list(members), np.asarray(groups, dtype=np.int32)
        buf, offs = bytearray(b"N"), []
        for s in self.tmpls + self.members:
            offs.append(len(buf))
            buf += s + b"N"
        self.arena = np.frombuffer(bytes(buf) + bytes(64), dtype=np.uint8)
        self.tmpl_off = np.array(offs[:len(self.tmpls)], dtype=np.int64)
        self.member_off = np.array(offs[len(self.tmpls):], dtype=np.int64)
        self.tmpl_len = np.array([len(s) for s in self.tmpls], dtype=np.int32)
        self.member_len = np.array([len(s) for s in self.members], dtype=np.int32)
        self._dev = None

    def host(self, band, tmpl_counts=1, table=TABLE, strand=None, votes=False):
        return cs.round_host(self.tmpls, self.members, self.groups, band, 30, tmpl_counts=tmpl_counts, qual_table=table, member_strand=strand,
                             return_votes=votes)

    def device(self, al, band, tmpl_counts=1, table=TABLE, strand=None):
        import torch
        if self._dev is None:
            self._dev = torch.from_numpy(self.arena.copy()).cuda()
        kw = {} if table is None else dict(qual_table=table)
        if strand is not None:
            kw["member_strand"] = strand
        return al.consensus_round(self._dev, self.tmpl_off, self.tmpl_len, self.member_off, self.member_len, self.groups, band, 30,
                                  tmpl_counts=tmpl_counts, **kw)


def same(got, want, what=""):
    assert np.array_equal(got.status, want.status), (what, "status")
    assert np.array_equal(got.distance, want.distance), (what, "distance")
    assert np.array_equal(got.voters, want.voters), (what, "voters", got.voters.tolist(), want.voters.tolist())
    assert np.array_equal(got.lens, want.lens), (what, "lengths", got.lens.tolist(), want.lens.tolist())
    assert got.cons.tobytes() == want.cons.tobytes(), (what, "consensus")
    if want.qual is None:
        assert got.qual is None, what
    else:
        assert got.qual is not None and got.qual.dtype == np.uint8 and got.qual.shape == got.cons.shape, what
        diff = np.nonzero(got.qual != want.qual)[0]
        assert diff.size == 0, (what, "qualities differ at", diff[:8].tolist(), got.qual[diff[:8]].tolist(), want.qual[diff[:8]].tolist())


def split_margins(r, G):
    """A model Round made with MARGIN and return_votes -> (margins of the emitted columns, margins of the emitted slots): a slot
    is emitted iff twice its sum exceeds the voters, a column unless deletion leads alone; output order as pc_consensus.h."""
    cols, slots, at = [], [], 0
    for g in range(G):
        v, voters = r.votes[g].astype(np.int64), int(r.voters[g])
        la = (v.size - 4 * cs.INS_SLOTS) // 21
        for p in range(la + 1):
            for s in range(cs.INS_SLOTS):
                k = 5 * la + (p * cs.INS_SLOTS + s) * 4
                if 2 * int(v[k:k + 4].sum()) > voters:
                    slots.append(int(r.qual[at]))
                    at += 1
            if p < la and int(v[5 * p:5 * p + 4].max()) >= int(v[5 * p + 4]):
                cols.append(int(r.qual[at]))
                at += 1
        assert at == int(r.lens[:g + 1].sum()), g
    return cols, slots


@pytest.fixture(scope="module")
def edges():
    """One group per template length, five members each; and the model at both bands and both tmpl_counts, computed once."""
    rng = random.Random(1820)
    tmpls, members, groups = [], [], []
    for g, la in enumerate(LENGTHS):
        t = "".join(rng.choice("ACGT") for _ in range(la)).encode()
        tmpls.append(t)
        if la <= 2:
            mine = [t, t, t[:-1], t + b"A", b"C" + t, b"N" * la, t.lower()]
        else:
            mine = _members(rng, t)
        members += mine
        groups += [g] * len(mine)
    case = Case(tmpls, members, groups)
    return case, {(band, counts): case.host(band, counts) for band in BANDS for counts in (0, 1)}


def test_the_model_shows_every_margin_the_issue_names(edges):
    case, _want = edges
    for band in BANDS:
        seen_cols, seen_slots = set(), set()
        for counts in (0, 1):
            r = case.host(band, counts, table=MARGIN, votes=True)
            assert (r.status[case.groups >= 2] == cs.ST_ACCEPTED).all(), (band, counts, r.status.tolist())       # the planned members all vote
            cols, slots = split_margins(r, len(case.tmpls))
            seen_cols |= set(cols)
            seen_slots |= set(slots)
        assert seen_cols >= {0, 1, 2, 3, 4, 5}, (band, sorted(seen_cols))
        assert seen_slots >= {0, 1}, (band, sorted(seen_slots))


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("tmpl_counts", [0, 1])
def test_qualities_equal_the_model(al, edges, band, tmpl_counts):
    case, want = edges
    w = want[(band, tmpl_counts)]
    assert w.lens.min() >= 1 and len(set(w.qual.tolist())) >= 5          # margins 0 .. 3 and 5, or 0 .. 4 and 6
    same(case.device(al, band, tmpl_counts), w, (band, tmpl_counts))


def test_without_a_table_the_call_is_todays(al, edges):
    case, want = edges
    plain = case.device(al, 8, 1, table=None)
    assert plain.qual is None
    w = want[(8, 1)]
    same(plain, cs.Round(w.cons, w.lens, w.status, w.distance, w.voters, None), "no table")
    again = case.device(al, 8, 1)                                # and the call with a table leaves the same bytes beside the qualities
    assert again.cons.tobytes() == plain.cons.tobytes() and np.array_equal(again.lens, plain.lens)


def test_mixed_strands_equal_the_model(al, edges):
    case, _want = edges
    strand = (np.arange(len(case.members)) % 3 == 1).astype(np.uint8)
    flipped = Case(case.tmpls, [cs.reverse_complement(m.upper()) if s else m for m, s in zip(case.members, strand)],
                   case.groups)
    for counts in (0, 1):
        w = flipped.host(8, counts, strand=strand)
        assert (w.status == cs.ST_ACCEPTED).sum() > 30
        same(flipped.device(al, 8, counts, strand=strand), w, ("strands", counts))
    same(flipped.device(al, 8, 1, strand=np.zeros(len(case.members), dtype=np.uint8)), flipped.host(8, 1), "all of strand 0")


def test_the_clamp_decides_above_255(al):
    tmpl = b"ACGTTGCA"
    case = Case([b"ACGTAC", tmpl, b"GGATCC"], [b"ACGTAC"] * 2 + [tmpl] * 300 + [b"GGATCC", b"GGTTCC"], [0] * 2 + [1] * 300 + [2] * 2)
    for counts in (0, 1):
        w = case.host(8, counts)
        assert w.voters[1] == 300 + counts and w.qual[6:14].tolist() == [int(TABLE[255])] * 8 and int(TABLE[255]) != int(TABLE[300 % 256])
        same(case.device(al, 8, counts), w, ("clamp", counts))


def test_a_bad_table_launches_nothing(al, edges):
    import torch
    case, want = edges
    bad = TABLE.copy()
    bad[200] = 94
    with pytest.raises(RuntimeError, match="bad argument"):
        case.device(al, 8, 1, table=bad)
    # straight at the entry point: an entry above 93, and exactly one of the two pointers NULL; nothing is written
    sub = Case(case.tmpls[:2], case.members[:14], case.groups[:14])
    arena = torch.from_numpy(sub.arena.copy()).cuda()
    d_off, d_len, d_grp = (torch.from_numpy(x).cuda() for x in (sub.member_off, sub.member_len, sub.groups))
    first = np.array([0, 7, 14], dtype=np.int64)
    cons = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    qual = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    lens = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    voters = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((14, 2), -7, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = np.ascontiguousarray(TABLE)
    for tab, q in ((bad.ctypes.data, qual.data_ptr()), (None, qual.data_ptr()), (good.ctypes.data, None)):
        rc = al.lib.pc_consensus_round_quality(al._ctx, arena.data_ptr(), arena.data_ptr(), sub.tmpl_off.ctypes.data, sub.tmpl_len.ctypes.data,
                                               first.ctypes.data, 2, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), None, 14, 8, 30, 65535, 1,
                                               cons.data_ptr(), lens.data_ptr(), voters.data_ptr(), out.data_ptr(), None, None, stream, tab, q)
        assert rc == BAD_ARG
    al.sync()
    for t, fill in ((cons, 7), (qual, 7), (lens, -7), (voters, -7), (out, -7)):
        assert (t.cpu().numpy() == fill).all()
    # both NULL: the call is pc_consensus_round_stranded
    rc = al.lib.pc_consensus_round_quality(al._ctx, arena.data_ptr(), arena.data_ptr(), sub.tmpl_off.ctypes.data, sub.tmpl_len.ctypes.data,
                                           first.ctypes.data, 2, d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr(), None, 14, 8, 30, 65535, 1,
                                           cons.data_ptr(), lens.data_ptr(), voters.data_ptr(), out.data_ptr(), None, None, stream, None, None)
    assert rc == 0
    al.sync()
    w = want[(8, 1)]
    assert lens.cpu().numpy()[:2].tolist() == w.lens[:2].tolist() and (qual.cpu().numpy() == 7).all()
    same(case.device(al, 8, 1), w, "after the refusals")


# ---- the rounds and the runner on the library ---------------------------------------------------------------------------------
def _copy(rng, tmpl, rate):
    out = []
    for ch in tmpl.decode():
        r = rng.random()
        if r < rate:
            continue
        if r < 2 * rate:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if rng.random() < rate else ch)
    return "".join(out).encode()


def test_two_rounds_through_call_groups(al):
    import torch
    rng = random.Random(1821)
    reads, groups, strands = [], [], []
    for g in range(6):
        original = "".join(rng.choice("ACGT") for _ in range(260)).encode()
        mine = []
        for k in range(5 + g % 3):
            mine.append(len(reads))
            minus = (g + k) % 2
            copy = _copy(rng, original, 0.05)
            reads.append(cs.reverse_complement(copy) if minus else copy)
            strands.append(minus)
        groups.append((g + 1, "KEY%d" % g, mine))
    off = np.concatenate([[0], np.cumsum([len(r) + 3 for r in reads])])[:-1].astype(np.int64)
    arena = np.frombuffer(b"".join(r + b"NNN" for r in reads) + bytes(64), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    dev_arena = torch.from_numpy(arena.copy()).cuda()
    table = cs.quality_table()
    for kw in (dict(read_strand=strands), dict(read_strand=strands, rounds=1)):
        host = cs.call_groups(groups, arena, off, lens, band=16, qual_table=table, **kw)
        dev = cs.call_groups(groups, arena, off, lens, band=16, qual_table=table, aligner=al, dev_arena=dev_arena, device="cuda", **kw)
        assert dev == host
        assert all(r["status"] == cs.CALLED and len(r["quality"]) == r["length"] for r in host)
        assert cs.fastq_text(dev) == cs.fastq_text(host) and cs.report_text(dev) == cs.report_text(host)
    assert any(strands[g[2][cs.template([lens[r] for r in g[2]])]] for g in groups), "no template read of strand 1: the reversal is not exercised"
    # without strands: the reads of strand 1 turned back first
    plain = [cs.reverse_complement(r) if s else r for r, s in zip(reads, strands)]
    arena = np.frombuffer(b"".join(r + b"NNN" for r in plain) + bytes(64), dtype=np.uint8)
    host = cs.call_groups(groups, arena, off, lens, band=16, rounds=3, qual_table=table)
    dev = cs.call_groups(groups, arena, off, lens, band=16, rounds=3, qual_table=table, aligner=al, dev_arena=torch.from_numpy(arena.copy()).cuda(),
                         device="cuda")
    assert dev == host and max(r["rounds"] for r in host) >= 2
    assert len({q for r in host for q in r["quality"]}) >= 4


def test_runner_writes_the_fastq_the_host_route_writes(tmp_path):
    from porechop_amd import runner
    from tests import consensus_case as ccase
    from tests import umi_runner_case
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(ccase.build()))
    opts = runner.Options()
    opts.check_reads = 3
    files = {}
    for tag, kw in (("library", {}), ("stand_in", dict(aligner=ccase.ConsensusAligner()))):
        out, fq, tsv = tmp_path / ("out_%s.fastq" % tag), tmp_path / ("cons_%s.fastq" % tag), tmp_path / ("cons_%s.tsv" % tag)
        res = runner.run(str(inp), output=str(out), options=opts, adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, umi=True,
                         umi_consensus_fastq=str(fq), umi_consensus_report=str(tsv), **kw)
        files[tag] = (fq.read_text(), tsv.read_text(), out.read_bytes(), [r["quality"] for r in res.consensus])
    assert files["library"] == files["stand_in"]
    assert files["library"][0].count("\n+\n") == 2 and files["library"][3][2:] == [None, None]
    assert sorted(set(files["library"][3][0])) == [25, 56] and sorted(set(files["library"][3][1])) == [10, 41]       # (tests/test_consensus_quality_cpu.py)
