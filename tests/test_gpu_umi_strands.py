"""Both strands of a molecule on the MI355X: pc_umi_neighbours_stranded / Aligner.umi_neighbours(strands=True)
(csrc/pc_umi_groups.hip) against umi_groups.neighbours_host(strands=True), and pc_consensus_round_stranded /
Aligner.consensus_round(member_strand=...) (csrc/pc_consensus.hip) against consensus.round_host(member_strand=...) -- both models
are checked against plain string code in tests/test_umi_strands_cpu.py.  Everything must be EQUAL.  The neighbours model runs
once per key set at max_dist 64 (d and flip of a pair do not depend on max_dist: every smaller max_dist is a filter of those
rows); the consensus model once per band and strand vector."""
import ctypes
import random

import numpy as np
import pytest

from porechop_amd import consensus as cs
from porechop_amd import umi_groups as ug

pytestmark = pytest.mark.gpu

N_ALL = 513                     # two tiles of 256 and a ragged third of one key: diagonal and off-diagonal blocks
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    from tests.umigen import SCHEMES
    a = porechop_amd.Aligner(["ACGTACGTACGT"], SCHEMES["default"])
    yield a
    a.close()


# ---- neighbours ----------------------------------------------------------------------------------------------------------------------
def _mutate(rng, key, edits, longest):
    k = list(key)
    for _ in range(edits):
        kind, at = rng.randrange(3), rng.randrange(len(k) + 1)
        if kind == 0 and k:
            k[min(at, len(k) - 1)] = rng.choice("ACGT")
        elif kind == 1 and len(k) < longest:
            k.insert(at, rng.choice("ACGT"))
        elif k:
            del k[min(at, len(k) - 1)]
    return "".join(k)


def _keys(name):
    """513 keys: seeded originals, each followed by a copy and a MIRROR of a copy 0 .. 3 edits away; a self-mirror key with a
    neighbour, and the tie (AATT is its own mirror: d_same == d_mirror against anything)."""
    longest = {"short": 32, "mixed": 64}[name]
    lengths = {"short": [0, 1, 22, 22, 31, 32, 32], "mixed": [0, 1, 31, 32, 33, 44, 63, 64, 64]}[name]
    rng = random.Random(longest)
    keys = ["AATT", "AAAT", "ACGT" * (longest // 4), "ACGT" * (longest // 4 - 1) + "ACGA"]
    while len(keys) < N_ALL:
        original = "".join(rng.choice("ACGT") for _ in range(rng.choice(lengths)))
        keys += [original, _mutate(rng, original, rng.randrange(4), longest), rc(_mutate(rng, original, rng.randrange(4), longest))]
    keys = keys[:N_ALL]
    rng.shuffle(keys)
    return keys


class KeySet:
    def __init__(self, name):
        self.keys = _keys(name)
        self.planes, self.lens = ug.pack(self.keys)
        self.all = ug.neighbours_host(self.planes, self.lens, 64, strands=True)        # the model, once
        self.plain = ug.neighbours_host(self.planes, self.lens, 64)
        assert self.all.shape == (N_ALL * (N_ALL - 1) // 2, 4)

    def want(self, max_dist, n=N_ALL):
        a = self.all
        return a[(a[:, 1] < n) & (a[:, 2] <= max_dist)]

    def want_plain(self, max_dist):
        return self.plain[self.plain[:, 2] <= max_dist]

    def device(self, n=N_ALL):
        import torch
        return (torch.from_numpy(np.ascontiguousarray(self.planes[:n]).view(np.int64)).cuda(),
                torch.from_numpy(np.ascontiguousarray(self.lens[:n])).cuda())


@pytest.fixture(scope="module")
def sets():
    made = {}

    def get(name):
        if name not in made:
            made[name] = KeySet(name)
        return made[name]
    return get


def test_a_key_and_its_mirror(al):
    import torch
    for key in ("ACGGATCCGTAAGCTTGGATTCAC", "ACGGATCCGTAAGCTTGGATTCACACGGATCCGTAAGCTTGGATTCAC", "A", "ACGTACGTACGTACGTACGTACGTACGTACGTA"):
        planes, lens = ug.pack([key, rc(key)])
        got = al.umi_neighbours(torch.from_numpy(planes.view(np.int64)).cuda(), torch.from_numpy(lens).cuda(), 2, strands=True)
        assert got.is_cuda and str(got.dtype) == "torch.int32"
        assert got.cpu().numpy().tolist() == [[0, 1, 0, 1]], key
    # a self-mirror key beside itself: the tie is flip 0; two empty keys
    planes, lens = ug.pack(["ACGT", "ACGT", "", ""])
    got = al.umi_neighbours(torch.from_numpy(planes.view(np.int64)).cuda(), torch.from_numpy(lens).cuda(), 0, strands=True)
    assert got.cpu().numpy().tolist() == [[0, 1, 0, 0], [2, 3, 0, 0]]


@pytest.mark.parametrize("name", ["short", "mixed"])
def test_stranded_neighbours_equal_the_model(sets, al, name, monkeypatch):
    ks = sets(name)
    assert ks.lens.max() == (32 if name == "short" else 64) and ks.lens.min() == 0        # one run per Word instantiation
    want2 = ks.want(2)
    assert (want2[:, 3] == 1).sum() >= 50 and (want2[:, 3] == 0).sum() >= 50               # asserted on the model: not vacuous
    i, j = ks.keys.index("AATT"), ks.keys.index("AAAT")
    assert [min(i, j), max(i, j), 1, 0] in want2.tolist()                                  # the tie
    i, j = sorted((ks.keys.index("ACGT" * (ks.lens.max() // 4)), ks.keys.index("ACGT" * (ks.lens.max() // 4 - 1) + "ACGA")))
    assert [i, j, 1, 0] in want2.tolist()                                                  # the self-mirror key and its neighbour
    planes, lens = ks.device()
    for max_dist in (0, 1, 2, 5):
        got = al.umi_neighbours(planes, lens, max_dist, strands=True).cpu().numpy()
        want = ks.want(max_dist)
        assert got.shape == want.shape and np.array_equal(got, want), (name, max_dist)
    for n in (2, 255, 256, 257, 512):
        p, l = ks.device(n)
        assert np.array_equal(al.umi_neighbours(p, l, 2, strands=True).cpu().numpy(), ks.want(2, n)), (name, n)
    # the unstranded call on the same keys returns what it returns today; the stranded rows with flip 0 are rows of it
    plain = al.umi_neighbours(planes, lens, 2).cpu().numpy()
    assert np.array_equal(plain, ks.want_plain(2))
    kept = want2[want2[:, 3] == 0][:, :3]
    assert {tuple(r) for r in kept.tolist()} <= {tuple(r) for r in plain.tolist()}
    # without the prunes: the same rows (the variable is read per call)
    monkeypatch.setenv("PC_UMI_NO_PRUNE", "1")
    for max_dist in (0, 2):
        assert np.array_equal(al.umi_neighbours(planes, lens, max_dist, strands=True).cpu().numpy(), ks.want(max_dist)), (name, max_dist)
    monkeypatch.delenv("PC_UMI_NO_PRUNE")
    # the route of the rule: kernel_order in, the caller's numbering out
    assert np.array_equal(ug.neighbours(ks.planes, ks.lens, 2, al, strands=True), want2)


def test_a_cap_below_found(sets, al):
    import torch
    ks = sets("mixed")
    planes, lens = ks.device()
    want = ks.want(3)
    cap = want.shape[0] // 3
    assert cap > 50
    pairs = torch.full((cap + 8, 4), -7, dtype=torch.int32, device="cuda")
    found = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    rc_ = al.lib.pc_umi_neighbours_stranded(al._ctx, planes.data_ptr(), lens.data_ptr(), N_ALL, 64, 3, pairs.data_ptr(), cap, found.data_ptr(),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0
    al.sync()
    assert int(found.item()) == want.shape[0]                               # exact, whatever fitted
    rows = pairs.cpu().numpy()
    assert (rows[cap:] == -7).all()                                         # nothing behind the cap
    written = {tuple(r) for r in rows[:cap].tolist()}
    assert len(written) == cap and written <= {tuple(r) for r in want.tolist()}
    assert np.array_equal(al.umi_neighbours(planes, lens, 3, cap=cap, strands=True).cpu().numpy(), want)


# ---- the pile-up ---------------------------------------------------------------------------------------------------------------------
BANDS = [1, 31, 32, 64, 96, 127]        # one, one, two, three, four and four cells of a row to a lane


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _resize(rng, tmpl, lb):
    """A member of exactly lb bases made from the template: bases dropped or inserted at random places, a few substituted --
    by N, lower case and U among others."""
    s = list(tmpl)
    while len(s) > lb:
        del s[rng.randrange(len(s))]
    while len(s) < lb:
        s.insert(rng.randrange(len(s) + 1), rng.choice("ACGT"))
    for _ in range(1 + len(s) // 12):
        s[rng.randrange(len(s))] = rng.choice("ACGTNacgu")
    return "".join(s)


def _materialise(stored):
    """The reverse complement of stored bytes as a string routine of this file: upper case, U as T, anything else N."""
    table = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A"}
    return "".join(table.get(ch.upper(), "N") for ch in reversed(stored))


class Pile:
    """Templates of 1, 255, 256, 257 and 1 100 bases; members at the edges of the two staging windows (1 024 bases for the
    rows, 256 for the walk), one member twice its template's length per group.  `as_read` is what the pile-up must see; a member
    of strand 1 lies in the arena as the reverse complement of that."""
    PLAN = [(1, [1, 2]), (255, [1, 255, 1023, 510]), (256, [256, 257, 1024, 512]), (257, [255, 1025, 1300, 514]), (1100, [1023, 1300, 2200])]

    def __init__(self):
        rng = random.Random(1919)
        self.tmpls, self.as_read, self.groups = [], [], []
        for g, (la, lbs) in enumerate(self.PLAN):
            t = _seq(rng, la)
            self.tmpls.append(t)
            for lb in lbs:
                self.as_read.append(_resize(rng, t, lb))
                self.groups.append(g)
        self.M = len(self.as_read)
        self.models = {}

    def stored(self, strand):
        """The members as they lie in the arena: strand-1 members reverse-complemented (their N stay N, their letters keep
        their case and U its name where the complement allows: a u read as the complement of a)."""
        out = []
        for s, st in zip(self.as_read, strand):
            if not st:
                out.append(s)
                continue
            keep = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "u", "c": "g", "g": "c", "u": "a", "N": "N"}
            out.append("".join(keep[ch] for ch in reversed(s)))
        return out

    def model(self, band, pct, strand):
        key = (band, pct, tuple(strand))
        if key not in self.models:
            self.models[key] = cs.round_host([t.encode() for t in self.tmpls], [s.encode() for s in self.stored(strand)], self.groups, band, pct,
                                             return_votes=True, member_strand=strand)
        return self.models[key]

    def device(self, al, band, pct, members, strand):
        import torch
        rng = random.Random(band)
        buf, offs = bytearray(_seq(rng, 7).encode()), []
        for s in self.tmpls + members:
            offs.append(len(buf))
            buf += s.encode() + _seq(rng, 3).encode()
        arena = torch.from_numpy(np.frombuffer(bytes(buf) + bytes(64), dtype=np.uint8).copy()).cuda()
        G = len(self.tmpls)
        return al.consensus_round(arena, np.array(offs[:G], dtype=np.int64), np.array([len(t) for t in self.tmpls], dtype=np.int32),
                                  np.array(offs[G:], dtype=np.int64), np.array([len(s) for s in members], dtype=np.int32),
                                  np.array(self.groups, dtype=np.int32), band, pct, return_votes=True,
                                  member_strand=None if strand is None else np.array(strand, dtype=np.uint8))


@pytest.fixture(scope="module")
def pile():
    return Pile()


def same(got, want, what=""):
    assert np.array_equal(got.status, want.status), (what, "status", got.status.tolist(), want.status.tolist())
    assert np.array_equal(got.distance, want.distance), (what, "distance", got.distance.tolist(), want.distance.tolist())
    assert np.array_equal(got.voters, want.voters), (what, "voters")
    assert len(got.votes) == len(want.votes)
    for g, (a, b) in enumerate(zip(got.votes, want.votes)):
        assert np.array_equal(a, b), (what, "votes of group", g, np.nonzero(a != b)[0][:8].tolist())
    assert np.array_equal(got.lens, want.lens), (what, "lengths", got.lens.tolist(), want.lens.tolist())
    assert got.cons.tobytes() == want.cons.tobytes(), (what, "consensus")


def test_the_stored_members_hold_what_they_claim(pile):
    mixed = [m % 2 for m in range(pile.M)]
    stored = pile.stored([1] * pile.M)
    assert any("N" in s for s in stored) and any("u" in s for s in stored) and any(set(s) & set("acg") for s in stored)
    for s, back in zip(pile.as_read, stored):
        assert cs.reverse_complement_codes(cs.codes(back.encode())).tolist() == cs.codes(s.encode()).tolist()
        assert cs.codes(_materialise(back).encode()).tolist() == cs.codes(s.encode()).tolist()
    assert sorted({len(s) for s in stored}) == [1, 2, 255, 256, 257, 510, 512, 514, 1023, 1024, 1025, 1300, 2200]
    assert 0 < sum(mixed) < pile.M


@pytest.mark.parametrize("band", BANDS)
def test_reverse_complemented_members_equal_the_model(al, pile, band):
    pct = 100                                   # whatever stays inside the band is accepted and walked
    for name, strand in (("all 1", [1] * pile.M), ("mixed", [m % 2 for m in range(pile.M)])):
        want = pile.model(band, pct, strand)
        if band >= 31:                          # asserted on the model: long members are walked, not only rejected
            accepted = [len(pile.as_read[m]) for m in range(pile.M) if want.status[m] == cs.ST_ACCEPTED]
            assert {1023, 1024, 1025, 1300} <= set(accepted), (band, sorted(accepted))
        stored = pile.stored(strand)
        got = pile.device(al, band, pct, stored, strand)
        same(got, want, (band, name))
        # the same members lying reverse-complemented in the arena, strand 0
        flat = [_materialise(s) if st else s for s, st in zip(stored, strand)]
        same(pile.device(al, band, pct, flat, [0] * pile.M), want, (band, name, "materialised"))
    # strand 0 throughout is pc_consensus_round: NULL, and an array of zeros
    null = pile.device(al, band, 30, pile.as_read, None)
    same(pile.device(al, band, 30, pile.as_read, [0] * pile.M), null, (band, "zeros against NULL"))
    same(null, pile.model(band, 30, [0] * pile.M), (band, "NULL against the model"))


def test_call_groups_with_a_minus_template_read(al):
    import torch
    rng = random.Random(77)
    seqs, strand, groups = [], [], []
    for g in range(3):
        orig = _seq(rng, 300 + 17 * g)
        reads = []
        for k in range(5):
            s = list(orig)
            for _ in range(6):
                s[rng.randrange(len(s))] = rng.choice("ACGT")
            minus = (k + g) % 2 == 0 or k == 2                     # all of one length: read 2 of each group is the round-1 template
            reads.append(len(seqs))
            seqs.append(rc("".join(s)) if minus else "".join(s))
            strand.append(int(minus))
        groups.append((g + 1, "K%d" % g, reads))
    arena = np.frombuffer("".join(seqs).encode() + bytes(64), dtype=np.uint8).copy()
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    want = cs.call_groups(groups, arena, off, lens, band=16, rounds=2, read_strand=strand)
    got = cs.call_groups(groups, arena, off, lens, band=16, rounds=2, read_strand=strand, aligner=al, dev_arena=torch.from_numpy(arena).cuda(),
                         device="cuda")
    assert got == want
    assert all(r["status"] == "called" and r["minus"] >= 2 and r["used"] == 5 for r in want)
    assert max(r["rounds"] for r in want) == 2
