"""The prefilter over reads held at 2 bits per base for EVERY adapter list and bound (pc_prefilter_packed_any): pieces the
seed stage cannot cover, adapters with a letter that is not a base and overflowing candidate lists run the exhaustive
kernel over the plane (prefilter_packed_kernel).  Its mask equals the byte route's bit for bit on reads and adapters made of
A/C/G/T, is a superset of it otherwise, and never drops a pair within the oracle's bound; the pipeline keeps its reads
packed at a threshold the seed stage does not cover when ScanParams.packed_total is set, and only then."""
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from porechop_amd.io import pack_reads
from tests.pairgen import mutate

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y_TOP, Y_BOTTOM = "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"


def nine_adapters():
    rng = random.Random(5)
    return [Y_TOP, Y_BOTTOM] + ["".join(rng.choice("ACGT") for _ in range(m)) for m in (4, 10, 24, 30, 33, 38, 70)]


def _packed_plane(arr, dev):
    pk, exc = pack_reads(arr)
    plane = torch.zeros(pk.size + 64, dtype=torch.uint8, device=dev)
    plane[:pk.size] = torch.from_numpy(pk).to(dev)
    return plane, (torch.from_numpy(exc).to(dev) if exc.size else None), exc


class Batch:
    """Reads back to back: the byte arena, the plane, offsets (the same numbers index bytes and bases) and lengths."""

    def __init__(self, reads, dev):
        self.reads = reads
        self.arr = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
        self.lens = np.array([len(r) for r in reads], dtype=np.int32)
        self.offs = np.concatenate([[0], np.cumsum(self.lens[:-1], dtype=np.int64)]).astype(np.int64)
        self.d_off, self.d_len = torch.from_numpy(self.offs).to(dev), torch.from_numpy(self.lens).to(dev)
        self.plane, self.d_exc, self.exc = _packed_plane(self.arr, dev)
        self.arena = torch.from_numpy(np.concatenate([self.arr, np.full(64, ord("N"), np.uint8)])).to(dev)
        self.max_len = int(self.lens.max())

    def both(self, al, ids, ks, arena=None):
        m_bytes = al.prefilter_mask(self.arena if arena is None else arena, self.d_off, self.d_len, self.max_len, ids, ks)
        m_plane = al.prefilter_mask_packed(self.plane, self.d_off, self.d_len, self.max_len, ids, ks, total=True)
        al.sync()
        assert m_plane is not None
        return m_bytes.cpu().numpy(), m_plane.cpu().numpy()


def bits_of(mask, na):
    return ((mask[:, :, None] >> np.arange(32)[None, None, :]) & 1).reshape(mask.shape[0], -1)[:, :na].T.astype(bool)      # [na, n]


def acgt_reads(adapters):
    """~1 500 reads of A/C/G/T at every length class and start residue, copies with 0..k edits at column 0, at the last
    column and across the chunk borders (512 i: 5 chunks of 512 columns at this many windows and 2 500 columns), and one
    copy cut in two by a read boundary."""
    from tests.test_gpu_prefilter import make_cases
    lengths = [0, 1, 5, 15, 16, 17, 63, 64, 65, 100, 150, 600, 2500]
    reads = [r.upper().replace("-", "A") for r in make_cases(1, 1450, lengths, adapters, alphabet="ACGT")]
    rng = random.Random(77)
    for ad in adapters:
        for rate in (0.0, 0.08, 0.15):
            body = "".join(rng.choice("ACGT") for _ in range(2500))
            spots = [0, 2500 - len(ad)] + [512 * i - len(ad) // 2 for i in (1, 2, 3, 4)] + [512 * 2 - 1, 512 * 3 - len(ad) + 1]
            r = list(body)
            for s in spots[rng.randrange(2)::2]:                 # (every other spot: copies far enough apart to stay separate)
                mut = mutate(rng, ad, rate)
                r[s:s + len(mut)] = mut
            reads.append("".join(r)[:2500])
    # Y_TOP's first half ends one read, its second half starts the next: it must not count for either
    split_at = len(reads)
    reads.append("".join(rng.choice("ACGT") for _ in range(300)) + Y_TOP[:14])
    reads.append(Y_TOP[14:] + "".join(rng.choice("ACGT") for _ in range(300)))
    return reads, split_at


def test_mask_equals_the_byte_route_for_every_group_shape_and_threshold(oracle):
    import porechop_amd
    dev = torch.device("cuda")
    adapters = nine_adapters()
    reads, split_at = acgt_reads(adapters)
    b = Batch(reads, dev)
    assert set("".join(reads)) <= set("ACGT") and b.exc.size == 0
    assert len(set((b.offs % 64).tolist())) == 64                # window starts at every residue of the 64-base block
    dist = {j: oracle.min_edits_many(b.arr, b.offs, b.lens, ad) for j, ad in enumerate(adapters) if len(ad) <= 32}
    al = porechop_amd.Aligner(adapters)
    try:
        assert al.prefilter_mask_packed(b.plane, b.d_off, b.d_len, b.max_len, list(range(9)), [al.max_edits(len(a), 85.0) for a in adapters]) is None
        for thr in (85.0, 80.0, 70.0, 90.0):
            # 9 adapters = 11 pieces at 85 % (the 70-mer is cut in three): groups of 8 + 4; the sub-lists of 1, 2, 3, 5, 6 and 7
            # adapters (one piece each; at 70 % the 33-mer is two) give 1, 2, 4, 4 + 1, 4 + 2 and 8 pieces per lane
            for ids in (list(range(9)), [3], [0, 4], [1, 2, 4], [0, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]):
                ks = [al.max_edits(len(adapters[j]), thr) for j in ids]
                a, p = b.both(al, ids, ks)
                assert np.array_equal(a, p), (thr, ids, int((a != p).sum()))
                got = bits_of(p, len(ids))
                for col, (j, k) in enumerate(zip(ids, ks)):
                    if j in dist:
                        want = (dist[j] <= k) & (b.lens > 0)
                        assert np.array_equal(got[col], want), (thr, ids, j, k, np.nonzero(got[col] != want)[0][:5])
                if ids[0] == 0 and thr == 90.0:                  # the copy cut in two by a read boundary
                    assert dist[0][split_at] > ks[0] and dist[0][split_at + 1] > ks[0]
                    assert not got[0][split_at] and not got[0][split_at + 1]
        # "do not filter this adapter": its bit is set exactly on the non-empty windows
        ids = list(range(9))
        ks = [al.max_edits(len(a), 85.0) for a in adapters]
        ks[2], ks[7] = -1, -1
        a, p = b.both(al, ids, ks)
        assert np.array_equal(a, p)
        got = bits_of(p, 9)
        assert np.array_equal(got[2], b.lens > 0) and np.array_equal(got[7], b.lens > 0)
        assert np.array_equal(got[0], (dist[0] <= ks[0]) & (b.lens > 0))
    finally:
        al.close()


def test_reads_with_letters_that_are_not_bases_are_scanned_as_the_plane_holds_them(oracle):
    import porechop_amd
    from tests.test_gpu_prefilter import make_cases
    dev = torch.device("cuda")
    adapters = nine_adapters()
    rng = random.Random(4)
    reads = []
    for r in make_cases(2, 600, [40, 150, 1000, 2500], adapters, alphabet="ACGTN-"):
        if rng.random() < 0.3:
            r = "".join(c.lower() if rng.random() < 0.3 else ("U" if c == "T" and rng.random() < 0.3 else c) for c in r)
        reads.append(r)
    b = Batch(reads, dev)
    assert b.exc.size > 100
    al = porechop_amd.Aligner(adapters)
    try:
        as_plane = al.unpack_device(b.plane, int(b.arr.size), None)      # no exception list: 'A' where the read held a non-base
        ids = list(range(9))
        for thr in (85.0, 90.0):
            ks = [al.max_edits(len(a), thr) for a in adapters]
            a_plane, p = b.both(al, ids, ks, arena=as_plane)
            assert np.array_equal(a_plane, p), (thr, int((a_plane != p).sum()))
            a_true, _ = b.both(al, ids, ks)
            assert np.all((a_true & ~p) == 0), thr                        # nothing the byte route keeps is dropped
            got = bits_of(p, 9)
            for j, (ad, k) in enumerate(zip(adapters, ks)):
                d = oracle.min_edits_many(b.arr, b.offs, b.lens, ad)
                assert not ((d <= k) & (b.lens > 0) & ~got[j]).any(), (thr, ad)
    finally:
        al.close()


def test_adapters_with_an_n_are_taken_with_the_n_as_a_wildcard(oracle):
    import porechop_amd
    from tests.test_gpu_prefilter import make_cases
    dev = torch.device("cuda")
    adapters = ["ACGTNNACGTTTGACCAGTNAC", Y_TOP[:10] + "N" + Y_TOP[11:]]
    reads = [r.upper() for r in make_cases(6, 800, [0, 30, 150, 700, 2500], adapters + [Y_TOP], alphabet="ACGTN")]
    b = Batch(reads, dev)
    al = porechop_amd.Aligner(adapters)
    try:
        for thr in (90.0, 85.0):
            ks = [al.max_edits(len(a), thr) for a in adapters]
            assert al.prefilter_mask_packed(b.plane, b.d_off, b.d_len, b.max_len, [0, 1], ks) is None       # the old entry point says no
            a, p = b.both(al, [0, 1], ks)
            assert np.all((a & ~p) == 0), thr
            got = bits_of(p, 2)
            assert got.any(axis=1).all() and not got.all(axis=1).any()
            for j, (ad, k) in enumerate(zip(adapters, ks)):
                d = oracle.min_edits_many(b.arr, b.offs, b.lens, ad)
                assert int(((d <= k) & (b.lens > 0)).sum()) > 20
                assert not ((d <= k) & (b.lens > 0) & ~got[j]).any(), (thr, ad)
    finally:
        al.close()


def test_ragged_lengths_with_a_length_hint():
    import porechop_amd
    from tests.test_gpu_prefilter import make_cases
    dev = torch.device("cuda")
    adapters = nine_adapters()
    reads = [r.upper().replace("-", "A") for r in make_cases(3, 300, [100, 3000, 70000], adapters, alphabet="ACGT")]
    b = Batch(reads, dev)
    al = porechop_amd.Aligner(adapters)
    try:
        al.set_length_hint(3000)
        ks = [al.max_edits(len(a), 85.0) for a in adapters]
        a, p = b.both(al, list(range(9)), ks)
        assert np.array_equal(a, p), int((a != p).sum())
        assert 50 < int((p != 0).any(axis=1).sum())
    finally:
        al.close()


# ---- a candidate list that overflows: redone by the exhaustive kernel over the plane ------------------------------------
def overflow_masks():
    """The batch of tests/test_gpu_prefilter_deferred.py (poly-A reads against a low-complexity adapter) at 90 %: the mask of
    an immediate call and the one of a deferred call followed, if the list overflowed, by the repeat call."""
    import porechop_amd
    from tests.test_gpu_prefilter import make_cases
    rng = random.Random(5)
    adapters = [Y_TOP, Y_BOTTOM, "".join(rng.choice("ACGT") for _ in range(24)), "".join(rng.choice("ACGT") for _ in range(32)),
                "AAAAAAAAAAAAAAAAAAAAAAAA"]
    reads = [r.replace("-", "A") for r in make_cases(31, 1500, [0, 5, 17, 150, 151, 600, 2500], adapters)] + ["A" * 3000, "ACGT" * 500]
    b = Batch(reads, torch.device("cuda"))
    al = porechop_amd.Aligner(adapters)
    try:
        ids = list(range(len(adapters)))
        ks = [al.max_edits(len(a), 90.0) for a in adapters]
        byte_mask, immediate = b.both(al, ids, ks)
        al.prefilter_defer_count(True)
        try:
            deferred = al.prefilter_mask_packed(b.plane, b.d_off, b.d_len, b.max_len, ids, ks, total=True)
        finally:
            al.prefilter_defer_count(False)
        al.sync()
        overflowed = al.prefilter_overflowed()
        if overflowed:
            deferred = al.prefilter_mask_packed(b.plane, b.d_off, b.d_len, b.max_len, ids, ks, total=True)
            al.sync()
        return byte_mask, immediate, deferred.cpu().numpy(), overflowed
    finally:
        al.close()


_OVERFLOW_CHILD = r"""
import hashlib, sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_packed_total import overflow_masks
byte_mask, immediate, deferred, overflowed = overflow_masks()
assert overflowed, "a 64-entry candidate list did not overflow"
assert np.array_equal(immediate, byte_mask) and np.array_equal(deferred, immediate)
print("CHILD_OK", hashlib.sha1(immediate.tobytes()).hexdigest(), int((immediate != 0).sum()))
"""


def test_an_overflowing_candidate_list_is_redone_over_the_plane():
    byte_mask, immediate, deferred, overflowed = overflow_masks()        # without the cap
    assert not overflowed and np.array_equal(immediate, byte_mask) and np.array_equal(deferred, immediate)
    r = subprocess.run([sys.executable, "-c", _OVERFLOW_CHILD % REPO], env=dict(os.environ, PC_PF_SEED_CAP="64"), capture_output=True,
                       text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert "filtered by the exhaustive kernel" in r.stderr
    digest, nonzero = r.stdout.split("CHILD_OK")[1].split()[:2]
    assert digest == hashlib.sha1(immediate.tobytes()).hexdigest() and int(nonzero) > 100


# ---- the pipeline: reads stay packed at a threshold the seed stage does not cover -----------------------------------------
def test_pipeline_keeps_reads_packed_at_threshold_85_only_when_asked_to():
    from porechop_amd.panel import load_panel
    from porechop_amd.pipeline import DeviceReads, Pipeline, ScanParams
    from tests.pairgen import synthetic_read
    rng = random.Random(9)
    reads = []
    for i in range(3000):
        r = synthetic_read(rng, rng.choice([40, 300, 900, 2500, 9000]), Y_TOP if rng.random() < 0.9 else None,
                           Y_BOTTOM if rng.random() < 0.5 else None, (Y_BOTTOM + Y_TOP) if i % 9 == 0 else None)
        r = list(r)
        for _ in range(rng.choice([0, 0, 1, 4, 40])):
            r[rng.randrange(len(r))] = rng.choice("NnX-RYacgtUu")
        reads.append("".join(r))
    arr = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    dev = torch.device("cuda")
    pk, exc = pack_reads(arr)

    def run(pl, rd):
        bs, be = pl.phase_a(rd, torch.arange(min(rd.n, 1000), device=dev))
        matching = pl.matching_sets(bs, be)
        st, et = pl.phase_b(rd, matching)
        hits = pl.phase_c(rd, st, et, matching, prefilter=True)
        pl.aligner.sync()
        return (bs.cpu(), be.cpu(), st.cpu(), et.cpu(), hits.read.cpu(), hits.adapter.cpu(), hits.start.cpu(), hits.end.cpu())

    def packed_reads(pl):
        return DeviceReads.packed_only(pl.aligner, torch.from_numpy(pk).to(dev), arr.size, torch.from_numpy(exc).to(dev),
                                       torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev))

    pl = Pipeline(load_panel(), ScanParams(middle_threshold=85.0, packed_total=True), device=dev)
    try:
        as_bytes = DeviceReads(torch.from_numpy(np.concatenate([arr, np.full(64, ord("N"), np.uint8)])).to(dev),
                               torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev))
        want = run(pl, as_bytes)
        as_packed = packed_reads(pl)
        got = run(pl, as_packed)
        stats = dict(pl.stats)
    finally:
        pl.close()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert want[4].numel() > 100
    assert as_packed.arena is None and "packed_route_refused" not in stats
    assert 0 < stats["bases_unpacked_after_prefilter"] < 0.5 * int(arr.size)          # only the survivors became bytes
    # the default is untouched: at 85 % the same reads are unpacked whole, and counted as a refusal
    pl = Pipeline(load_panel(), ScanParams(middle_threshold=85.0), device=dev)
    try:
        as_packed = packed_reads(pl)
        got = run(pl, as_packed)
        stats = dict(pl.stats)
    finally:
        pl.close()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert stats.get("packed_route_refused", 0) >= 1 and as_packed.arena is not None
