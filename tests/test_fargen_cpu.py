"""The far-offset placements of tests/fargen.py, checked on the host: the boundaries 2^31 and 2^32 fall where the GPU tests
(tests/test_gpu_far_offsets.py) need them, the four placements hold the same strings, and -- with the oracle alone --
the batch is not degenerate: every DP adapter has hits, and at every prefilter threshold a fair share of the pairs lies
on either side of the bound."""
import numpy as np
import pytest

from tests import fargen
from tests.fargen import B31, B32, PLACEMENTS


@pytest.fixture(scope="module")
def far():
    dp, nine, long200, every = fargen.far_adapters()
    layout, acgt = fargen.make_layout(fargen.SEED, every)
    return layout, acgt, dp, nine, long200


def arena_bytes(layout, block=None):
    """The written bytes of the arena as {first byte: bytes} and a reader over them (anything else is unwritten)."""
    images = dict(layout.image(name, block) for name in PLACEMENTS)

    def read(off, n):
        for first, data in images.items():
            if first <= off and off + n <= first + len(data):
                return data[off - first:off - first + n]
        raise AssertionError("bytes %d..%d are not written" % (off, off + n))
    return images, read


def test_block_shape(far):
    layout, acgt, *_ = far
    b = layout.block
    assert b.n == 133 and len(b.data) < 64 * 1024
    base = sorted(b.len[[i for i in range(b.n) if i not in b.sub]].tolist())
    assert base == sorted(fargen.LENGTHS)
    assert {1, 3, 16, 17, 149, 150, 151, 700, 2500} == set(base) and base.count(150) > 100
    text = b.data.decode("latin-1")
    assert set(text) >= set("ACGTN-acgtUu") and set(acgt.data.decode("latin-1")) == set("ACGT")
    assert sum(1 for p in b.planted if p) >= 60
    # back to back, the two sub-windows tile the designated one
    d, (x, y) = b.designated, b.sub
    rest = [i for i in range(b.n) if i not in b.sub]
    assert np.array_equal(b.off[rest][1:], (b.off[rest] + b.len[rest])[:-1]) and b.off[0] == 0
    assert b.off[x] == b.off[d] and b.off[y] == b.off[x] + b.len[x] and b.len[x] + b.len[y] == b.len[d] >= 300
    assert b.reads[x] + b.reads[y] == b.reads[d]
    dis = b.disjoint
    assert np.all(b.off[dis][1:] >= (b.off[dis] + b.len[dis])[:-1])


@pytest.mark.parametrize("name,boundary", [("cross31", B31), ("cross32", B32)])
def test_boundary_inside_the_designated_copy_and_between_two_windows(far, name, boundary):
    layout, _, dp, *_ = far
    b = layout.block
    off = b.off + layout.start[name]
    d, (x, y) = b.designated, b.sub
    lo, hi = int(off[d]) + b.copy[0], int(off[d]) + b.copy[1]
    assert lo < boundary < hi - 1, (lo, boundary, hi)           # strictly inside the copy: bases of it on both sides
    assert off[d] < boundary < off[d] + b.len[d]
    assert off[x] + b.len[x] - 1 == boundary - 1 and off[y] == boundary     # one window ends in the byte before, the next starts on it
    assert b.len[x] > 0 and b.len[y] > 0
    # the copy is one of the first DP adapter, recognisably
    cp = b.reads[d][b.copy[0]:b.copy[1]]
    assert len(cp) >= 16 and sum(1 for p, q in zip(cp, dp[0]) if p == q) >= 8


def test_beyond32_starts_take_every_residue(far):
    layout, *_ = far
    s = layout.start["beyond32"]
    assert s > B32 and s % 2 == 1
    off = layout.block.off + s
    assert len(set((off % 64).tolist())) == 64 and len(set((off % 16).tolist())) == 16
    assert off.min() >= B32


def test_placements_fit_the_arena_and_do_not_touch(far):
    layout, *_ = far
    spans = []
    for name in PLACEMENTS:
        first, data = layout.image(name)
        assert first % 64 == 0 and first >= 0 and first + len(data) + 64 <= fargen.ARENA_BYTES
        if name != "near":
            assert len(layout.lead[name]) >= fargen.LEAD
        assert len(layout.tail[name]) == fargen.TAIL
        spans.append((first, first + len(data)))
    assert all(spans[i][1] + 4096 < spans[i + 1][0] for i in range(3))
    leads = [layout.lead[n][:fargen.LEAD] for n in PLACEMENTS[1:]]
    tails = [layout.tail[n] for n in PLACEMENTS]
    assert len(set(leads)) == 3 and len(set(tails)) == 4


def test_the_four_placements_slice_to_identical_strings(far):
    layout, acgt, *_ = far
    for block in (layout.block, acgt):
        _, read = arena_bytes(layout, block)
        for name in PLACEMENTS:
            rows = layout.rows(name)
            got = [read(int(o), int(l)).decode("latin-1") for o, l in zip(layout.win_off[rows], layout.win_len[rows])]
            assert got == block.reads, name
    assert layout.win_off.dtype == np.int64 and layout.win_len.dtype == np.int32
    assert layout.win_off.shape[0] == 4 * layout.block.n


def test_exceptions_on_both_sides_of_two_to_the_32(far):
    from porechop_amd.io import unpack_reads_host
    layout, acgt, *_ = far
    packed, exc = layout.packed_images()
    assert exc.dtype == np.int64 and np.all(np.diff(exc) > 0)
    assert (exc < B31).any() and ((exc > B31) & (exc < B32)).any() and (exc >= B32).any()
    first, data = layout.image("cross32")
    inside = exc[(exc >= layout.start["cross32"]) & (exc < layout.start["cross32"] + len(layout.block.data))]
    assert (inside < B32).any() and (inside >= B32).any()               # inside the block too, not only in the margins
    # each image unpacks to its own canonical bytes
    for name in PLACEMENTS:
        at, pk, e = packed[name]
        first, data = layout.image(name)
        assert at * 4 == first and (at + pk.size) <= fargen.PLANE_BYTES - 64
        canon = unpack_reads_host(pk, len(data), e - first)
        raw = np.frombuffer(data, dtype=np.uint8)
        is_base = np.isin(raw, np.frombuffer(b"ACGTUacgtu", dtype=np.uint8))
        assert np.all(canon[~is_base] == ord("N")) and not np.any(canon[is_base] == ord("N"))
    # the A/C/G/T variant has no exception inside a block
    _, exc_same = layout.packed_images(acgt)
    for name in PLACEMENTS:
        s = layout.start[name]
        assert not ((exc_same >= s) & (exc_same < s + len(acgt.data))).any()


def test_every_dp_adapter_has_hits(far, oracle):
    """Per adapter at least 20 windows whose reference alignment has a positive score and a non-empty path, and at least
    8 whose full-adapter identity reaches 70 % (planted copies that survived their mutations)."""
    layout, _, dp, nine, long200 = far
    b = layout.block
    schemes = [(ad, fargen.SCORES) for ad in dp + [long200]] + [(dp[0], (3, -6, -5, -5)), (dp[2], (3, -6, -5, 0))]
    for ad, scores in schemes:
        hits = good = 0
        for r in b.reads:
            x = oracle.align_raw(r, ad, scores)
            if not x.failed and x.score > 0 and x.path_len > 0:
                hits += 1
                good += x.full_len > 0 and 100.0 * x.full_matches / x.full_len >= 70.0
        assert hits >= 20, (len(ad), scores, hits)
        assert good >= 8 or ad is long200, (len(ad), scores, good)


@pytest.mark.parametrize("thr", fargen.THRESHOLDS)
def test_prefilter_bound_splits_the_batch(far, oracle, thr):
    """Of the (window, adapter) pairs of the nine prefilter adapters, between 10 % and 90 % lie within the bound.  The share
    is taken over the pairs, not per adapter: 133 windows of which every second is planted hold 15-16 copies of each of
    the 13 sequences, a third of them drawn at rate 0.15 and beyond the bound at 90 %, so no adapter but the 4-mer can
    have 10 % of the windows within it; and at 70 % the 4- and the 10-mer lie within one and four edits of nearly every
    window of 16 bases or more.  Per adapter of at most 32 bases -- where the mask is checked exactly -- the floor is what
    the planting guarantees: of the 10 copies drawn at rates 0 and 0.05, at most two lost to a cut at the edge of their
    ~50 columns or to a third edit, so at least 8 windows within the bound; and at least the 3 windows too short to
    hold anything (1, 1 and 3 bases against a bound below the adapter's length) beyond it."""
    import porechop_amd
    lib = porechop_amd.load_library()
    layout, acgt, _, nine, _ = far
    for block in (layout.block, acgt):
        arr = np.frombuffer(block.data, dtype=np.uint8)
        shares = []
        for ad in nine:
            k = int(lib.pc_prefilter_max_edits(len(ad), thr))
            within = (oracle.min_edits_many(arr, block.off, block.len, ad) <= k) & (block.len > 0)
            shares.append(float(within.mean()))
            if len(ad) <= 32:
                assert 8 <= int(within.sum()) <= block.n - 3, (thr, len(ad), k, int(within.sum()))
        assert 0.10 <= float(np.mean(shares)) <= 0.90, (thr, shares)
