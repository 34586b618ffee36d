"""Seeded batches for the score-floor tests (TEST INFRASTRUCTURE, CPU only).

A batch is 193 whole reads -- three 64-pair tiles plus one lane -- of random bases with planted copies of the four middle
adapters of two panel sets (1D^2 part 2: 33 | 30, SQK-NSK007: 28 | 22) carrying 0..8 substitutions / indels, so that the
full-adapter identities of the planted copies straddle --middle_threshold.  Six of the reads are built, with the oracle, so
that their best score against one adapter is EXACTLY that adapter's score bound, or the bound minus one: the two sides of
the comparison the library makes.  Everything a test compares against is computed here once per batch and never changed."""
import random
import types

import numpy as np

SCORES = (3, -6, -5, -2)
SETS = ("1D^2 part 2", "SQK-NSK007")          # dual jobs (33 | 30) and (28 | 22)
N_READS = 193
NO_FLOOR = -2 ** 31


def middle_adapters():
    """[(name, sequence)] x 4: start and end sequence of the two sets, set by set (the order phase_c scans them in)."""
    from tests.golden_io import load_panel
    by_name = {a["name"]: a for a in load_panel()}
    out = []
    for s in SETS:
        out += [tuple(by_name[s]["start"]), tuple(by_name[s]["end"])]
    assert [len(a[1]) for a in out] == [33, 30, 28, 22]
    return out


def score_bound(m, threshold, scores=SCORES):
    """Pipeline.identity_score_bound itself (not a restatement), without a device."""
    from porechop_amd.pipeline import Pipeline
    return Pipeline.identity_score_bound(types.SimpleNamespace(p=types.SimpleNamespace(scores=scores)), m, threshold)


def edit(rng, seq, k):
    """seq with k random substitutions / deletions / insertions."""
    s = list(seq)
    for _ in range(k):
        i = rng.randrange(len(s))
        x = rng.random()
        if x < 0.5:
            s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
        elif x < 0.75:
            del s[i]
        else:
            s.insert(i, rng.choice("ACGT"))
    return "".join(s)


def random_bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def read_with_score(oracle, rng, adapter, want, length, tries=20000):
    """A read of `length` random bases with one edited copy of `adapter` whose best score against it is exactly `want`."""
    for _ in range(tries):
        copy = edit(rng, adapter, rng.randint(1, 8))
        if rng.random() < 0.4:
            copy = copy[:rng.randint(len(copy) // 2, len(copy))]
        body = random_bases(rng, length - len(copy))
        pos = rng.randint(40, len(body) - 40)
        rd = body[:pos] + copy + body[pos:]
        if oracle.align_raw(rd, adapter, SCORES).score == want:
            return rd
    raise AssertionError("no read with score %d found" % want)


class Batch:
    """reads (strings), and per (adapter, read): the oracle's record [rs, re, as, ae, score, matches, aligned_len, full_len] in the
    library's layout, its score, its full identity.  `floors(threshold)`: the four score bounds."""

    def __init__(self, oracle, seed, ragged, threshold=90.0):
        rng = random.Random(seed)
        self.ads = middle_adapters()
        self.threshold = threshold
        seqs = [a[1] for a in self.ads]
        self.bounds = [score_bound(len(s), threshold) for s in seqs]
        assert all(b is not None for b in self.bounds)
        reads = []
        for i in range(N_READS):
            ln = rng.randint(300, 2000) if ragged else 1000
            if i in (0, N_READS - 1) and ragged:
                ln = 300 if i == 0 else 2000
            body = random_bases(rng, ln)
            if rng.random() < 0.6:                       # one to three planted copies, 0..8 edits each
                for _ in range(rng.randint(1, 3)):
                    a, k = rng.randrange(len(seqs)), rng.randint(0, 8)
                    if a == 0 and k == 0:
                        k = 1                            # (the one exact copy of adapter 0 is read 63's: lane63_floors)
                    copy = edit(rng, seqs[a], k)
                    pos = rng.randint(0, len(body))
                    body = (body[:pos] + copy + body[pos:])[:ln]
            if i == 63:
                body = body[:100] + seqs[0] + body[100 + len(seqs[0]):]
            reads.append(body)
        # the two sides of the comparison, for three of the adapters: score == bound and score == bound - 1
        self.exact = []
        for k, a in enumerate((0, 2, 3)):
            for d in (0, 1):
                slot = 5 + 31 * (2 * k + d)              # spread over the tiles
                reads[slot] = read_with_score(oracle, rng, seqs[a], self.bounds[a] - d, len(reads[slot]))
                self.exact.append((a, slot, self.bounds[a] - d))
        self.reads = reads
        self.lens = np.array([len(r) for r in reads], dtype=np.int32)
        self.offs = np.concatenate([[0], np.cumsum(self.lens[:-1].astype(np.int64))]).astype(np.int64)
        self.arena = np.frombuffer(("".join(reads)).encode() + b"N" * 64, dtype=np.uint8).copy()
        ad_arena = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        ad_len = np.array([len(s) for s in seqs], dtype=np.int32)
        ad_off = np.concatenate([[0], np.cumsum(ad_len[:-1].astype(np.int64))]).astype(np.int64)
        n, A = N_READS, len(seqs)
        o = oracle.align_many(self.arena, np.tile(self.offs, A), np.tile(self.lens, A), ad_arena, np.repeat(ad_off, n), np.repeat(ad_len, n),
                              SCORES).reshape(A, n, 9)
        self.score = o[:, :, 4].astype(np.int64)                                   # [A, n]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.full = np.round(100.0 * o[:, :, 7] / o[:, :, 8], 6)
        self.full = np.where(o[:, :, 0] == -1, 0.0, np.nan_to_num(self.full))
        for a, slot, want in self.exact:
            assert self.score[a, slot] == want
        self.max_len = int(self.lens.max())
        self.typ_len = int(self.lens.mean())

    def below(self, floors):
        """[A, n] bool: the pairs a call with these four floors must leave untraced."""
        return self.score < np.array(floors, dtype=np.int64)[:, None]


def lane63_floors(batch):
    """Floors that leave exactly ONE pair of adapter 0's segment above them: the one of read 63 (lane 63 of the first tile as
    the pairs are handed over), and none of the other three adapters' pairs."""
    s = batch.score[0].copy()
    s[63] = -10 ** 6
    f0 = int(s.max()) + 1
    assert batch.score[0, 63] >= f0, "read 63 must score above every other read against adapter 0"
    return [f0] + [int(batch.score[a].max()) + 1 for a in (1, 2, 3)]
