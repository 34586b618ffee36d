"""slow_kernel and path_kernel against one another and the oracle, pair for pair (both run the cell of csrc/pc_cell.h).

Two schemes the packed kernels refuse whatever the adapter's length (6 * (match - mismatch) > 16000), so that the scan of
every pair runs slow_kernel, and that pcs::fits accepts: the default scheme times 1000 (affine) and a linear one
(gap_open == gap_extend).  Adapters of 1, 7, 8, 9 and 33 bases -- a row group of the packed trace partial, full and new.
305 windows of 0 to 60 bases, every length five times, each against an adapter its position picks: the empty window,
all-N windows, lower-case bytes, letters outside ACGT, and mutated copies of the adapters in either case.  The scan's
records (Aligner.align_pairs) equal those of Aligner.align_pairs_paths, both equal the oracle's, and every path passes
tests/pathcheck.py; no pair is left out.
"""
import random

import numpy as np
import pytest

from tests import pathcheck
from tests.pairgen import mutate

pytestmark = pytest.mark.gpu

ADAPTER_LENGTHS = (1, 7, 8, 9, 33)
SCHEMES = {"affine": (3000, -6000, -5000, -2000), "linear": (3000, -6000, -4000, -4000)}
NPAIRS = 305


class Cases:
    def __init__(self):
        rng = random.Random(950)
        self.adapters = ["".join(rng.choice("ACGT") for _ in range(m)) for m in ADAPTER_LENGTHS]
        self.pairs = []
        for k in range(NPAIRS):
            n, a = k % 61, (k // 61 + k) % 5
            kind = k % 7
            if kind == 0:
                body = "N" * n
            else:
                body = [rng.choice("ACGTACGTACGTNacgtU-X") for _ in range(n)]
                if kind >= 3:
                    cp = mutate(rng, self.adapters[a], rng.choice((0.0, 0.05, 0.15, 0.3)))[:n]
                    at = rng.randint(0, n - len(cp))
                    body[at:at + len(cp)] = cp
                body = "".join(body)
                if kind == 6:
                    body = body.lower()
            self.pairs.append((body, a))
        lengths = [len(r) for r, _ in self.pairs]
        assert sorted(set(lengths)) == list(range(61)) and lengths.count(0) == 5
        assert any(r and set(r) == {"N"} for r, _ in self.pairs) and any(r and r == r.lower() for r, _ in self.pairs)
        assert {(len(r) > 0, a) for r, a in self.pairs} >= {(True, a) for a in range(5)}
        self._want = {}

    def want(self, oracle, name):
        if name not in self._want:
            self._want[name] = [oracle.align_raw(r, self.adapters[a], SCHEMES[name]) for r, a in self.pairs]
        return self._want[name]


@pytest.fixture(scope="module")
def cases():
    return Cases()


@pytest.mark.parametrize("name", list(SCHEMES))
def test_scan_and_paths_agree_pair_for_pair(cases, oracle, name):
    import porechop_amd
    scheme = SCHEMES[name]
    assert (scheme[2] == scheme[3]) == (name == "linear")
    al = porechop_amd.Aligner(cases.adapters, scheme)
    try:
        for m in ADAPTER_LENGTHS:
            assert al.lib.pc_scores_supported(*scheme, m) == 0        # every pair of the scan runs the plain-int32 kernel
        scan = al.align_pairs(cases.pairs)
        recs, heads, strings = al.align_pairs_paths(cases.pairs)
    finally:
        al.close()
    want = cases.want(oracle, name)
    assert scan.shape == recs.shape == (NPAIRS, 8) and heads.shape == (NPAIRS, 4) and len(strings) == len(want) == NPAIRS
    for p, (read, a) in enumerate(cases.pairs):
        where = (name, p, read, cases.adapters[a])
        assert scan[p].tolist() == recs[p].tolist() == pathcheck.oracle_record(want[p]), where
        try:
            pathcheck.check_path(read, cases.adapters[a], scheme, recs[p], heads[p], strings[p], want[p])
        except AssertionError as e:
            raise AssertionError("%r: %s" % (where, e))
    # the data exercises something: all four operations, failed and empty alignments
    joined = "".join(strings)
    assert all(op in joined for op in "=XID")
    assert int((recs[:, 0] == -1).sum()) >= 5 and any(h[0] == 0 and r for h, (r, _) in zip(heads, cases.pairs))
