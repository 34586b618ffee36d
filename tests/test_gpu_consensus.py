"""The UMI consensus round on the MI355X (pc_consensus_round / Aligner.consensus_round, csrc/pc_consensus.hip) against the numpy
model consensus.round_host -- itself checked against hand-stated pile-ups in tests/test_consensus_cpu.py, and the rule's C++
against a full matrix in tests/test_consensus_host.py.  Everything must be EQUAL: votes, statuses, distances, voters, consensus
bytes and lengths.  The shapes are the smallest at which this kernel can go wrong: the band's edges against the template's
length, members at the band's limit on either side, the wave's and the slice's edges."""
import ctypes
import random

import numpy as np
import pytest

from porechop_amd import consensus as cs

pytestmark = pytest.mark.gpu

BAD_ARG = -3
BANDS = [1, 2, 8, 32, 64, 127]        # 32 and 127: two and four cells of a row to a lane (64: three)


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    from tests.umigen import SCHEMES
    a = porechop_amd.Aligner(["ACGTACGTACGT"], SCHEMES["default"])
    yield a
    a.close()


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def _resize(rng, tmpl, lb):
    """A member of exactly lb bases made from the template: bases dropped or inserted at random places, a few substituted."""
    s = list(tmpl.decode())
    while len(s) > lb:
        del s[rng.randrange(len(s))]
    while len(s) < lb:
        s.insert(rng.randrange(len(s) + 1), rng.choice("ACGT"))
    for _ in range(len(s) // 12):
        s[rng.randrange(len(s))] = rng.choice("ACGTNacgu")
    return "".join(s).encode()


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


class Case:
    """Templates and members laid into one arena (gap bytes between the sequences; `lead` bytes in front)."""

    def __init__(self, tmpls, members, groups, lead=0, gap=1, seed=0):
        rng = random.Random(seed)
        self.tmpls, self.members, self.groups = list(tmpls), list(members), np.asarray(groups, dtype=np.int32)
        buf, offs = bytearray(_seq(rng, lead, "ACGTN")), []
        for s in self.tmpls + self.members:
            offs.append(len(buf))
            buf += s + _seq(rng, gap, "ACGTN")
        self.arena = np.frombuffer(bytes(buf) + bytes(64), dtype=np.uint8)
        self.tmpl_off = np.array(offs[:len(self.tmpls)], dtype=np.int64)
        self.member_off = np.array(offs[len(self.tmpls):], dtype=np.int64)
        self.tmpl_len = np.array([len(s) for s in self.tmpls], dtype=np.int32)
        self.member_len = np.array([len(s) for s in self.members], dtype=np.int32)

    def host(self, band, pct, max_len=65535, tmpl_counts=1):
        return cs.round_host(self.tmpls, self.members, self.groups, band, pct, max_len, tmpl_counts, return_votes=True)

    def device(self, al, band, pct, max_len=65535, tmpl_counts=1, arena=None, shift=0, votes=True):
        import torch
        arena = torch.from_numpy(self.arena.copy()).cuda() if arena is None else arena
        return al.consensus_round(arena, self.tmpl_off + shift, self.tmpl_len, self.member_off + shift, self.member_len, self.groups, band, pct,
                                  max_len=max_len, tmpl_counts=tmpl_counts, return_votes=votes)


def same(got, want, what=""):
    assert np.array_equal(got.status, want.status), (what, "status", got.status.tolist(), want.status.tolist())
    assert np.array_equal(got.distance, want.distance), (what, "distance", got.distance.tolist(), want.distance.tolist())
    assert np.array_equal(got.voters, want.voters), (what, "voters")
    if want.votes is not None and got.votes is not None:
        assert len(got.votes) == len(want.votes)
        for g, (a, b) in enumerate(zip(got.votes, want.votes)):
            assert np.array_equal(a, b), (what, "votes of group", g, np.nonzero(a != b)[0][:8].tolist())
    assert np.array_equal(got.lens, want.lens), (what, "lengths", got.lens.tolist(), want.lens.tolist())
    assert got.cons.tobytes() == want.cons.tobytes(), (what, "consensus")


def _edge_case(band):
    """One group per template length at the band's edges; per group a member of every length at which the band's reach ends."""
    rng = random.Random(1800 + band)
    tmpls, members, groups = [], [], []
    for la in sorted({1, 2, band, band + 1, 2 * band + 1, 2 * band + 2, 300}):
        g = len(tmpls)
        t = _seq(rng, la)
        tmpls.append(t)
        reach = {(2 * band + 2) * la + 1} if la <= 2 else set()          # beyond about (2 band + 1) la no path stays inside the band
        for lb in sorted(({0, 1, la, la - 1, la + 1, la - band, la + band, la - band - 1, la + band + 1, 2 * la} | reach) - set(range(-400, 0))):
            members.append(_resize(rng, t, lb))
            groups.append(g)
        members += [b"N" * la, t, t.lower(), _copy(rng, t, 0.03), _copy(rng, t, 0.08)]         # all N; the template itself; a noisy copy
        groups += [g] * 5
    return Case(tmpls, members, groups, seed=band)


@pytest.mark.parametrize("band", BANDS)
def test_the_bands_edges_equal_the_model(al, band):
    case = _edge_case(band)
    for pct in (30, 100):
        want = case.host(band, pct)
        if pct == 100:          # asserted on the model: the case holds accepted and rejected members and a path that cannot stay inside
            assert (want.status == cs.ST_ACCEPTED).sum() > 20
        else:
            assert (want.status == cs.ST_REJECTED).sum() > 5 and (want.status == cs.ST_ACCEPTED).sum() > 10
        same(case.device(al, band, pct), want, (band, pct))
    assert (want.distance == cs.INF).sum() >= 2 and (want.status[want.distance == cs.INF] == cs.ST_REJECTED).all()
    # the template as an earlier consensus: it votes but is no voter
    same(case.device(al, band, 30, tmpl_counts=0), case.host(band, 30, tmpl_counts=0), (band, "tmpl_counts 0"))


@pytest.fixture(scope="module")
def crowd():
    """Groups of 1, 2, 63, 64, 65 and 257 members of about 40 bases, and its model at band 8."""
    rng = random.Random(257)
    tmpls, members, groups = [], [], []
    for g, n in enumerate([1, 2, 63, 64, 65, 257]):
        t = _seq(rng, 36 + g)
        tmpls.append(t)
        members += [_copy(rng, t, 0.06) for _ in range(n)]
        groups += [g] * n
    case = Case(tmpls, members, groups, seed=7)
    return case, case.host(8, 30)


def test_members_per_group(al, crowd):
    case, want = crowd
    assert want.voters.tolist()[:2] == [2, 3] and want.voters[5] > 200
    same(case.device(al, 8, 30), want)


def test_member_order_shuffled_gives_the_same_votes(al, crowd):
    case, want = crowd
    rng = random.Random(3)
    order = []
    for g in range(len(case.tmpls)):
        mine = [m for m in range(len(case.members)) if case.groups[m] == g]
        rng.shuffle(mine)
        order += mine
    assert order != sorted(order)
    shuffled = Case(case.tmpls, [case.members[m] for m in order], case.groups, seed=8)
    got = shuffled.device(al, 8, 30)
    for g in range(len(case.tmpls)):
        assert np.array_equal(got.votes[g], want.votes[g]), g
    assert got.cons.tobytes() == want.cons.tobytes() and np.array_equal(got.voters, want.voters)
    assert np.array_equal(got.distance, want.distance[order])


@pytest.fixture(scope="module")
def many():
    """130 groups of three or four members on templates of 90 .. 300 bases, and its model at band 8: the results of a prefix
    of the groups are a prefix of these."""
    rng = random.Random(130)
    tmpls, members, groups = [], [], []
    for g in range(130):
        t = _seq(rng, rng.choice([90, 150, 299, 300]))
        tmpls.append(t)
        n = 3 + g % 2
        members += [_copy(rng, t, 0.05) for _ in range(n)]
        groups += [g] * n
    case = Case(tmpls, members, groups, seed=9)
    return case, case.host(8, 30)


def _prefix(case, want, G):
    M = int((case.groups < G).sum())
    sub = Case(case.tmpls[:G], case.members[:M], case.groups[:M], seed=10)
    n = int(want.lens[:G].sum())
    return sub, cs.Round(want.cons[:n], want.lens[:G], want.status[:M], want.distance[:M], want.voters[:G], want.votes[:G])


@pytest.mark.parametrize("G", [1, 2, 65, 130])
def test_groups(al, many, G):
    sub, want = _prefix(*many, G)
    same(sub.device(al, 8, 30), want, G)
    same(sub.device(al, 8, 30, votes=False), want, (G, "the library's own votes"))


def test_slices_fall_inside_the_call(al, many, monkeypatch):
    """1 MB of scratch: a slice holds about a dozen of these groups (votes 4 * (21 la + 16), trace members * (la + 1) * 64), so
    the call is cut many times; a group of 50 members on 300 bases (988 KB) is a slice of its own; one of 60 is refused."""
    case, want = many
    rng = random.Random(50)
    t = _seq(rng, 300)
    big = [_copy(rng, t, 0.05) for _ in range(50)]
    G = len(case.tmpls)
    assert 4 * cs.votes_per_group(300) + 50 * 301 * 64 < (1 << 20) < 4 * cs.votes_per_group(300) + 60 * 301 * 64
    # the big group in the middle: slices before it, it alone, slices behind it
    half = 64
    M_half = int((case.groups < half).sum())
    groups = np.concatenate([case.groups[:M_half], np.full(50, half), case.groups[M_half:] + 1])
    mixed = Case(case.tmpls[:half] + [t] + case.tmpls[half:], case.members[:M_half] + big + case.members[M_half:], groups, seed=11)
    want_mixed = mixed.host(8, 30)
    monkeypatch.setenv("PC_CONSENSUS_SCRATCH_MB", "1")
    same(mixed.device(al, 8, 30), want_mixed, "debug votes")
    same(mixed.device(al, 8, 30, votes=False), want_mixed, "sliced votes")
    # above the budget: refused with the group's index, before anything is launched
    over = Case(case.tmpls[:3] + [t], case.members[:int((case.groups < 3).sum())] + big + big[:10],
                np.concatenate([case.groups[case.groups < 3], np.full(60, 3)]), seed=12)
    with pytest.raises(cs.OverBudget) as e:
        over.device(al, 8, 30)
    assert e.value.args[0] == 3
    monkeypatch.delenv("PC_CONSENSUS_SCRATCH_MB")
    same(case.device(al, 8, 30), want, "after the refusal")
    assert G == 130


def test_every_byte_alignment(al, many):
    sub, want = _prefix(*many, 4)
    for lead in range(16):
        placed = Case(sub.tmpls, sub.members, sub.groups, lead=lead, gap=lead % 3, seed=20 + lead)
        same(placed.device(al, 8, 30), want, lead)


def test_behind_byte_2_32_of_the_arena(al, many):
    import torch
    from tests import fargen
    free, _ = torch.cuda.mem_get_info()
    if free < (12 << 30):
        pytest.skip("less than 12 GB of device memory free (%.1f GB)" % (free / 2**30))
    sub, want = _prefix(*many, 6)
    block = torch.from_numpy(sub.arena.copy()).cuda()
    arena = torch.empty(fargen.ARENA_BYTES, dtype=torch.uint8, device="cuda")
    try:
        # one copy starts behind 2^32 at an odd byte; another lies across 2^32, which falls inside its third member
        for start in (fargen.BEYOND32_START, fargen.B32 - int(sub.member_off[2]) - 7):
            assert start + block.numel() < fargen.ARENA_BYTES
            arena[start:start + block.numel()] = block
            same(sub.device(al, 8, 30, arena=arena, shift=start), want, start)
    finally:
        del arena
        torch.cuda.empty_cache()


def test_refusals_launch_nothing(al, many):
    import torch
    sub, want = _prefix(*many, 2)
    for kw in (dict(band=0), dict(band=128), dict(band=-1), dict(max_len=0), dict(pct=-1), dict(pct=101), dict(tmpl_counts=2)):
        args = dict(band=8, pct=30, max_len=65535, tmpl_counts=1)
        args.update(kw)
        with pytest.raises(RuntimeError, match="bad argument"):
            sub.device(al, **args)
    zero = Case(sub.tmpls, sub.members, sub.groups, seed=1)
    zero.tmpl_len = zero.tmpl_len.copy()
    zero.tmpl_len[1] = 0
    with pytest.raises(RuntimeError, match="bad argument"):
        zero.device(al, 8, 30)
    # negative counts, straight at the entry point; nothing is written
    lens = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    dummy = torch.zeros(64, dtype=torch.int64, device="cuda")
    first = np.zeros(3, dtype=np.int64)
    for G, M in ((-1, 3), (2, -1)):
        rc = al.lib.pc_consensus_round(al._ctx, dummy.data_ptr(), dummy.data_ptr(), first.ctypes.data, first.ctypes.data, first.ctypes.data, G,
                                       dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), M, 8, 30, 65535, 1, dummy.data_ptr(), lens.data_ptr(),
                                       dummy.data_ptr(), dummy.data_ptr(), None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == BAD_ARG
    al.sync()
    assert (lens.cpu().numpy() == -7).all()
    # zero groups, zero members: nothing at all
    none = Case([], [], [], seed=2)
    got = none.device(al, 8, 30)
    assert got.lens.size == 0 and got.cons.size == 0 and got.status.size == 0
    alone = Case(sub.tmpls, [], [], seed=3)
    same(alone.device(al, 8, 30), alone.host(8, 30), "no members")
    same(sub.device(al, 8, 30), want, "after the refusals")


def test_a_length_above_max_len_is_reported_at_sync(al, many):
    sub, want = _prefix(*many, 3)
    assert max(len(t) for t in sub.tmpls) > 100
    with pytest.raises(RuntimeError):
        sub.device(al, 8, 30, max_len=100)
    long_member = Case(sub.tmpls[:1], [sub.members[0], sub.members[1] * 2], [0, 0], seed=4)
    with pytest.raises(RuntimeError):
        long_member.device(al, 8, 30, max_len=320)
    same(sub.device(al, 8, 30), want, "after the report")


# ---- the rounds and the runner on the library ---------------------------------------------------------------------------------
def _molecules(seed, n_groups, copies, length, rate):
    rng = random.Random(seed)
    reads, groups = [], []
    for g in range(n_groups):
        original = _seq(rng, length)
        mine = []
        for _ in range(copies + g % 3):
            mine.append(len(reads))
            reads.append(_copy(rng, original, rate))
        groups.append((g + 1, "KEY%d" % g, mine))
    return reads, groups


def test_two_rounds_through_call_groups(al):
    import torch
    reads, groups = _molecules(18, 9, 5, 260, 0.05)
    groups.append((10, "FEW", [len(reads)]))
    reads.append(b"ACGTACGT")
    off = np.concatenate([[0], np.cumsum([len(r) + 3 for r in reads])])[:-1].astype(np.int64)
    arena = np.frombuffer(b"".join(r + b"NNN" for r in reads) + bytes(64), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    host = cs.call_groups(groups, arena, off, lens, band=16, rounds=3)
    dev = cs.call_groups(groups, arena, off, lens, band=16, rounds=3, aligner=al, dev_arena=torch.from_numpy(arena.copy()).cuda(), device="cuda")
    assert dev == host
    assert [r["status"] for r in host] == [cs.CALLED] * 9 + [cs.FEW_READS]
    assert max(r["rounds"] for r in host) >= 2
    assert cs.fasta_text(dev) == cs.fasta_text(host) and cs.report_text(dev) == cs.report_text(host)


def test_runner_writes_the_consensus_the_host_route_writes(tmp_path):
    from porechop_amd import runner
    from tests import consensus_case as ccase
    from tests import umi_runner_case
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(ccase.build()))
    opts = runner.Options()
    opts.check_reads = 3
    out, fa, tsv = tmp_path / "out.fastq", tmp_path / "cons.fasta", tmp_path / "cons.tsv"
    res = runner.run(str(inp), output=str(out), options=opts, adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, umi=True,
                     umi_consensus=str(fa), umi_consensus_report=str(tsv))
    assert fa.read_text() == ccase.FASTA and tsv.read_text() == ccase.TSV
    assert [r["sequence"] for r in res.consensus] == ccase.SEQUENCES
    plain = tmp_path / "plain.fastq"
    runner.run(str(inp), output=str(plain), options=opts, adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, umi=True)
    assert out.read_bytes() == plain.read_bytes()
