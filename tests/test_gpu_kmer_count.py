"""The k-mer census kernels on the MI355X (csrc/pc_discover.hip: pc_kmer_count, pc_kmer_select) against the numpy model
(tests/kmer_model.py), for exact equality: window lengths across the chunk and overlap boundaries at odd arena offsets, the
alphabet, overlapping / empty / repeated window lists, contended counters, k = 13, the candidate list and its overflow
retry, argument checks."""
import numpy as np
import pytest

from tests import kmer_model as km

pytestmark = pytest.mark.gpu

BAD_ARG = -3                                   # PC_ERR_BAD_ARG (include/porechop_amd.h)


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    a = porechop_amd.Aligner(["ACGTACGTAC"])
    yield a
    a.close()


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def rand_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def lay_out(rng, windows, residues=(1, 3)):
    """The windows in one arena, window i at an offset that is residues[i % len] mod 4 -- odd by default -- with random
    BASES between them and behind the last: a byte read from outside a window would be counted."""
    parts, offs, pos = [], [], 0
    for i, w in enumerate(windows):
        gap = 5 + (residues[i % len(residues)] - (pos + 5)) % 4
        parts.append(rand_bases(rng, gap))
        pos += gap
        offs.append(pos)
        parts.append(bytes(w))
        pos += len(w)
    parts.append(rand_bases(rng, 64))
    arena = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return dev(arena), dev(np.array(offs, dtype=np.int64)), dev(np.array([len(w) for w in windows], dtype=np.int32))


def assert_table(counts, codes, cnt):
    """the device table's nonzero entries are exactly (codes ascending, cnt)"""
    import torch
    nz = torch.nonzero(counts).flatten()
    got_codes = nz.cpu().numpy()
    got = counts[nz].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(got_codes, codes), (got_codes[:8], codes[:8])
    assert np.array_equal(got, cnt), (got[:8], cnt[:8])


def census(al, windows, k, rng, **kw):
    arena, off, ln = lay_out(rng, windows, **kw)
    return al.kmer_count(arena, off, ln, k)


# ---- window lengths ---------------------------------------------------------------------------------------------------------
def lengths_for(k):
    return [0, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, 258, 1000]


@pytest.mark.parametrize("k", [4, 8, 12])
def test_window_lengths_across_chunk_and_overlap_boundaries(al, k):
    rng = np.random.default_rng(100 + k)
    every = []
    for n in lengths_for(k):
        windows = [rand_bases(rng, n), rand_bases(rng, n)]             # one at 1 mod 4, one at 3 mod 4
        assert_table(census(al, windows, k, rng), *km.count_sparse(windows, k))
        every += windows
    # ... and all of them in one call, at every residue
    assert_table(census(al, every, k, rng, residues=(0, 1, 2, 3, 3, 2, 1)), *km.count_sparse(every, k))


def test_chunk_boundaries_with_non_bases_around_them(al):
    """N's just before, on and after the 256th start of a long window: the k-mers dropped are the ones that cover them"""
    k = 12
    rng = np.random.default_rng(5)
    windows = []
    for at in (243, 244, 255, 256, 257, 267, 268, 511, 512, 523):
        w = bytearray(rand_bases(rng, 700))
        w[at] = ord("N")
        windows.append(bytes(w))
    assert_table(census(al, windows, k, rng), *km.count_sparse(windows, k))


# ---- alphabet ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 8, 12])
def test_a_non_base_removes_exactly_the_kmers_that_cover_it(al, k):
    rng = np.random.default_rng(k)
    base = rand_bases(rng, k + 2)
    whole = km.kmer_codes([base], k)
    assert whole.size == 3
    for ch in b"N-nX":
        for at in range(k + 2):
            w = bytearray(base)
            w[at] = ch
            codes, cnt = km.count_sparse([bytes(w)], k)
            assert codes.size == sum(1 for s in range(3) if not s <= at < s + k)      # the model itself: starts 0, 1, 2
            assert_table(census(al, [bytes(w)], k, rng), codes, cnt)


def test_u_is_t_and_lower_case_is_coded_like_upper_case(al):
    k = 8
    rng = np.random.default_rng(8)
    base = rand_bases(rng, 40)
    want = km.count_sparse([base], k)
    assert_table(census(al, [base.replace(b"T", b"U")], k, rng), *want)
    assert_table(census(al, [base.lower()], k, rng), *want)
    assert_table(census(al, [base.lower().replace(b"t", b"u")], k, rng), *want)
    mixed = bytes(c + 32 if i % 3 == 0 else c for i, c in enumerate(base))
    assert_table(census(al, [mixed], k, rng), *want)


def test_every_byte_value(al):
    """all 256 byte values between two runs of bases: the scans' byte -> code table, entry by entry"""
    k = 4
    rng = np.random.default_rng(256)
    for b in range(256):
        w = rand_bases(rng, 5) + bytes([b]) + rand_bases(rng, 5)
        assert_table(census(al, [w], k, rng), *km.count_sparse([w], k))


# ---- layout -------------------------------------------------------------------------------------------------------------------
def test_overlapping_windows_are_both_counted(al):
    """the start and the end window of a read shorter than end_size are the same bytes"""
    import torch
    k = 8
    rng = np.random.default_rng(9)
    reads = [rand_bases(rng, n) for n in (5, 8, 40, 149, 150, 151, 300)]
    arena, off, ln = lay_out(rng, reads)
    wl = torch.clamp(ln, max=150)
    end_off = off + (ln - wl).to(torch.int64)
    counts = al.kmer_count(arena, torch.cat([off, end_off]), torch.cat([wl, wl]), k)
    assert_table(counts, *km.count_sparse([r[:150] for r in reads] + [r[-150:] for r in reads], k))


def test_no_windows_leaves_the_table_untouched(al):
    import torch
    k = 8
    before = torch.arange(1 << (2 * k), dtype=torch.int32, device="cuda")
    table = before.clone()
    arena = dev(np.frombuffer(b"ACGTACGTACGTACGT", dtype=np.uint8))
    out = al.kmer_count(arena, torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), k,
                        counts=table)
    assert out is table and torch.equal(table, before)


def test_two_calls_into_one_table_equal_one_call(al):
    import torch
    k = 12
    rng = np.random.default_rng(12)
    windows = [rand_bases(rng, int(n)) for n in rng.integers(0, 400, size=300)]
    arena, off, ln = lay_out(rng, windows)
    one = al.kmer_count(arena, off, ln, k)
    two = al.kmer_count(arena, off[:120].contiguous(), ln[:120].contiguous(), k)
    assert al.kmer_count(arena, off[120:].contiguous(), ln[120:].contiguous(), k, counts=two) is two
    assert torch.equal(one, two)
    assert_table(one, *km.count_sparse(windows, k))


def test_window_beyond_two_to_the_31(al):
    """offsets are 64-bit: a window behind byte 2^31 of the arena"""
    import torch
    k = 8
    rng = np.random.default_rng(31)
    w = rand_bases(rng, 300)
    at = (1 << 31) + 101
    arena = torch.empty(at + 300 + 64, dtype=torch.uint8, device="cuda")
    arena[at - 64:] = ord("A")
    arena[at:at + 300] = dev(np.frombuffer(w, dtype=np.uint8))
    counts = al.kmer_count(arena, dev(np.array([at], dtype=np.int64)), dev(np.array([300], dtype=np.int32)), k)
    assert_table(counts, *km.count_sparse([w], k))


# ---- contention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 12])
@pytest.mark.parametrize("homopolymer", [False, True])
def test_one_window_listed_20000_times(al, k, homopolymer):
    rng = np.random.default_rng(20000)
    w = b"A" * 150 if homopolymer else rand_bases(rng, 150)
    arena, off, ln = lay_out(rng, [w])
    counts = al.kmer_count(arena, off.repeat(20000), ln.repeat(20000), k)
    codes, cnt = km.count_sparse([w], k)
    if homopolymer:
        assert codes.tolist() == [0] and cnt.tolist() == [150 - k + 1]
    assert_table(counts, codes, 20000 * cnt)


# ---- k = 13 -------------------------------------------------------------------------------------------------------------------
def test_k13(al):
    rng = np.random.default_rng(13)
    windows = [rand_bases(rng, 150) for _ in range(2000)]
    counts = census(al, windows, 13, rng)
    codes, cnt = km.count_sparse(windows, 13)
    assert int(counts.sum(dtype=__import__("torch").int64)) == 2000 * (150 - 13 + 1) == int(cnt.sum())
    assert_table(counts, codes, cnt)


# ---- the candidate list ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skewed(al):
    """a table with a wide spread of counts: 400 windows that share a 40-mer behind random bases (k = 8)"""
    k = 8
    rng = np.random.default_rng(88)
    shared = rand_bases(rng, 40)
    windows = [rand_bases(rng, int(rng.integers(0, 12))) + shared[:int(rng.integers(20, 41))] + rand_bases(rng, 60) for _ in range(400)]
    counts = census(al, windows, k, rng)
    return k, counts, km.count_dense(windows, k)


def test_candidates_equal_the_model_and_are_sorted(al, skewed):
    k, counts, model = skewed
    present = int(np.sort(model[model > 0])[-20])                  # a count that occurs
    for floor in (present, present + 1, 1):
        codes, cnt = al.kmer_candidates(counts, k, floor)
        want = np.nonzero(model >= floor)[0]
        assert codes.dtype == np.int64 and cnt.dtype == np.int64
        assert np.array_equal(np.sort(codes), want)
        assert np.array_equal(cnt, model[codes])
        order = np.lexsort((codes, -cnt))
        assert np.array_equal(order, np.arange(codes.size)), "count descending, then code ascending"
    assert want.size > 400                                          # (floor 1: ties by the hundred, so the code order is exercised)


def test_candidates_retry_after_an_overflow(al, skewed):
    k, counts, model = skewed
    full = al.kmer_candidates(counts, k, 2)
    assert full[0].size == int((model >= 2).sum()) > 7
    small = al.kmer_candidates(counts, k, 2, cap=7)
    assert np.array_equal(small[0], full[0]) and np.array_equal(small[1], full[1])
    empty = al.kmer_candidates(counts, k, int(model.max()) + 1, cap=0)
    assert empty[0].size == 0 and empty[1].size == 0


def test_raw_select_reports_the_full_number_and_writes_only_members(al, skewed):
    k, counts, model = skewed
    total = int((model >= 2).sum())
    codes, cnt, found = al.kmer_select(counts, k, 2, 7)
    assert int(found.item()) == total > 7
    codes, cnt = codes.cpu().numpy().astype(np.int64), cnt.cpu().numpy().astype(np.int64)
    assert len(set(codes.tolist())) == 7
    assert np.all(model[codes] >= 2) and np.array_equal(cnt, model[codes])
    _, _, none = al.kmer_select(counts, k, 2, 0)
    assert int(none.item()) == total


# ---- arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 14])
def test_k_out_of_range_is_refused_without_a_launch(al, k):
    import ctypes
    import torch
    arena = dev(np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8))
    off, ln = dev(np.array([0], dtype=np.int64)), dev(np.array([20], dtype=np.int32))
    table = torch.zeros(1 << 8, dtype=torch.int32, device="cuda")           # (smaller than any table these k would index)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert al.lib.pc_kmer_count(al._ctx, arena.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, k, table.data_ptr(), s) == BAD_ARG
    found = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert al.lib.pc_kmer_select(al._ctx, table.data_ptr(), k, 1, out.data_ptr(), out.data_ptr(), 4, found.data_ptr(), s) == BAD_ARG
    torch.cuda.synchronize()
    assert int(table.abs().sum()) == 0 and int(found.item()) == -5
    with pytest.raises(RuntimeError, match="bad argument"):
        al.kmer_count(arena, off, ln, k)
