"""insert_code_kernel on the MI355X (csrc/pc_discover.hip: pc_anchor_inserts) against the numpy model (tests/barcode_model.py),
element for element: hand-made records on every branch of the rule, every insert length and both sides, the alphabet, window
lists that overlap and repeat, a window behind byte 2^31, records of a real scan, argument checks."""
import numpy as np
import pytest

from tests import barcode_model as bm
from tests import kmer_model as km

pytestmark = pytest.mark.gpu

BAD_ARG = -3                                   # PC_ERR_BAD_ARG (include/porechop_amd.h)
LENGTHS = [1, 12, 24, 31, 32]


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    a = porechop_amd.Aligner([bm.A_S, bm.A_E])
    yield a
    a.close()


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def rand_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def lay_out(rng, windows):
    """The windows in one arena at odd offsets with random BASES between them and behind the last: a byte read from outside
    a window would change a code, not fault.  -> (arena, offsets, lengths) as numpy arrays"""
    parts, offs, pos = [], [], 0
    for i, w in enumerate(windows):
        gap = 33 + (i % 3)
        parts.append(rand_bases(rng, gap))
        pos += gap
        offs.append(pos)
        parts.append(bytes(w))
        pos += len(w)
    parts.append(rand_bases(rng, 64))
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(offs, dtype=np.int64), np.array([len(w) for w in windows], dtype=np.int32)


def record(read_start, read_end, ad_start, ad_end, matches, full_len, score=7, aligned_len=None):
    return [read_start, read_end, ad_start, ad_end, score, matches, full_len if aligned_len is None else aligned_len, full_len]


def both(al, arena, off, ln, records, anchor_len, side, min_identity, L):
    """kernel and model over the same arrays -> (kernel's codes, model's codes) as numpy arrays"""
    records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 8)
    got = al.anchor_inserts(dev(arena), dev(off), dev(ln), dev(records), anchor_len, side, min_identity=min_identity, insert_len=L)
    assert got.dtype == __import__("torch").int64 and got.is_cuda and tuple(got.shape) == (off.shape[0],)
    return got.cpu().numpy(), bm.anchor_inserts(arena, off, ln, records, anchor_len, side, min_identity, L)


# ---- every branch of the rule ---------------------------------------------------------------------------------------------
def rule_cases(L, side, m=30, wl=80):
    """(window length, record, anchored and inside?) for a window of wl bases and an anchor of m: one case per branch"""
    edge = dict(ad_start=0, ad_end=m - 1)
    inner = dict(read_start=L + 5, read_end=wl - L - 6)               # the insert well inside the window on either side

    def rec(matches=m, full_len=m, **kw):
        f = dict(edge, **inner)
        f.update(kw)
        return record(f["read_start"], f["read_end"], f["ad_start"], f["ad_end"], matches, full_len)
    cases = [
        (wl, rec(), True),
        (wl, [-1, 0, 0, 0, 0, 0, 0, 0], False),                                    # the failure record
        (wl, rec(read_start=-1), False),
        (wl, rec(matches=0, full_len=0), False),                                   # full_len 0 (0 >= 0 would pass the identity)
        (wl, rec(matches=3, full_len=4), True),                                    # 300 >= 75 * 4: exactly at min_identity
        (wl, rec(matches=2, full_len=4), False),                                   # one match below
        (wl, rec(matches=15, full_len=20), True),
        (wl, rec(matches=14, full_len=20), False),
        (wl, rec(matches=2 ** 30, full_len=2 ** 30 + 1), True),                    # products beyond 32 bits
        (wl, rec(matches=2 ** 29, full_len=2 ** 30 + 1), False),
        (wl, rec(ad_end=m - 2), side == 1),                                        # the inner edge of side 0
        (wl, rec(ad_end=m), side == 1),
        (wl, rec(ad_start=1), side == 0),                                          # the inner edge of side 1
        (wl, rec(read_end=-1), True),                                              # side 0: col == 0
        (wl, rec(read_end=-2), side == 1),                                         # side 0: col == -1
        (wl, rec(read_start=L), True),                                             # side 1: col == 0
        (wl, rec(read_start=L - 1), side == 0),                                    # side 1: col == -1
        (wl, rec(read_end=wl - L - 1), True),                                      # side 0: col + L == win_len
        (wl, rec(read_end=wl - L), side == 1),                                     # side 0: one beyond
        (wl, rec(read_start=wl), True),                                            # side 1: col + L == win_len
        (wl, rec(read_start=wl + 1), side == 0),                                   # side 1: one beyond
    ]
    for n in (0, 1, L - 1, L):                                                     # short windows: only L fits, at col 0
        cases.append((n, rec(read_end=-1, read_start=L), n == L))
    return cases


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("L", LENGTHS)
def test_every_branch_of_the_rule(al, L, side):
    rng = np.random.default_rng(100 * L + side)
    cases = rule_cases(L, side)
    arena, off, ln = lay_out(rng, [rand_bases(rng, n) for n, _, _ in cases])
    got, want = both(al, arena, off, ln, [r for _, r, _ in cases], 30, side, 75, L)
    for i, (n, r, inside) in enumerate(cases):
        # (at L = 32 the code fills the sign bit and 32 T's are -1: "some code came back" is asked of the model's bits)
        assert (want[i] != -1) == inside or L == 32, (i, n, r)
    assert np.array_equal(got, want), [(i, cases[i][1], int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:5]]
    # the codes are the window's bytes: the first case, spelled out
    n, r, _ = cases[0]
    col = r[1] + 1 if side == 0 else r[0] - L
    v = km.encode(bytes(arena[off[0] + col:off[0] + col + L]).decode())
    assert int(want[0]) == (v - (1 << 64) if v >= 1 << 63 else v)


def test_min_identity_0_and_100(al):
    rng = np.random.default_rng(7)
    recs = [record(0, 9, 0, 29, m, 30) for m in (0, 1, 29, 30)]
    arena, off, ln = lay_out(rng, [rand_bases(rng, 60) for _ in recs])
    for ident, anchored in ((0, [1, 1, 1, 1]), (100, [0, 0, 0, 1]), (97, [0, 0, 0, 1]), (96, [0, 0, 1, 1])):     # 29 of 30: 2900 < 2910
        got, want = both(al, arena, off, ln, recs, 30, 0, ident, 24)
        assert np.array_equal(got, want) and [int(x >= 0) for x in want] == anchored


# ---- n -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_numbers_of_windows(al, n):
    import torch
    rng = np.random.default_rng(n)
    L, m = 24, 30
    windows = [rand_bases(rng, int(k)) for k in rng.integers(0, 151, size=n)]
    arena, off, ln = lay_out(rng, windows)
    recs = np.zeros((n, 8), dtype=np.int32)
    for i in range(n):                                                 # records all over the place, most of them anchored
        rs = int(rng.integers(-1, 150))
        recs[i] = record(rs, rs + int(rng.integers(0, 40)), int(rng.integers(0, 8) == 0), m - 1 - int(rng.integers(0, 8) == 0),
                         int(rng.integers(20, 31)), 30)
    for side in (0, 1):
        got, want = both(al, arena, off, ln, recs, m, side, 75, L)
        assert np.array_equal(got, want)
        assert n < 200 or (0 < int((want >= 0).sum()) < n)
    if n == 0:
        assert al.anchor_inserts(dev(arena), dev(off), dev(ln), torch.zeros((0, 8), dtype=torch.int32, device="cuda"), m, 0).numel() == 0


# ---- alphabet ----------------------------------------------------------------------------------------------------------------
def test_every_byte_value_inside_an_insert(al):
    """all 256 byte values at the first, a middle and the last position of an insert: four bases in either case and U / u
    give the code, any other byte -1"""
    rng = np.random.default_rng(256)
    L = 12
    windows, want_base = [], []
    for b in range(256):
        for at in (0, 5, L - 1):
            w = bytearray(rand_bases(rng, 8 + L + 4))
            w[8 + at] = b
            windows.append(bytes(w))
            want_base.append(bytes([b]) in b"ACGTUacgtu")
    arena, off, ln = lay_out(rng, windows)
    recs = [record(2, 7, 0, 29, 30, 30)] * len(windows)
    got, want = both(al, arena, off, ln, recs, 30, 0, 75, L)
    assert np.array_equal(got, want) and [bool(x >= 0) for x in want] == want_base
    assert sum(want_base) == 3 * 10


def test_u_is_t_and_lower_case_is_coded_like_upper_case(al):
    rng = np.random.default_rng(8)
    base = rand_bases(rng, 60)
    mixed = bytes(c + 32 if i % 3 == 0 else c for i, c in enumerate(base))
    windows = [base, base.replace(b"T", b"U"), base.lower(), base.lower().replace(b"t", b"u"), mixed]
    arena, off, ln = lay_out(rng, windows)
    for side, r in ((0, record(3, 20, 0, 29, 28, 30)), (1, record(40, 59, 0, 29, 28, 30))):
        got, want = both(al, arena, off, ln, [r] * 5, 30, side, 75, 24)
        assert np.array_equal(got, want) and len(set(got.tolist())) == 1 and got[0] >= 0


# ---- layout ------------------------------------------------------------------------------------------------------------------
def test_overlapping_and_repeated_windows(al):
    """the start and the end window of a read shorter than end_size are the same bytes; one window listed many times"""
    rng = np.random.default_rng(9)
    reads = [rand_bases(rng, n) for n in (5, 24, 40, 149, 150, 151, 300)]
    arena, off, ln = lay_out(rng, reads)
    wl = np.minimum(ln, 150).astype(np.int32)
    woff = np.concatenate([off, off + (ln - wl), np.repeat(off[-1:], 300)])
    wlen = np.concatenate([wl, wl, np.repeat(wl[-1:], 300)])
    recs = [record(30, 35, 0, 29, 30, 30)] * 14 + [record(24 + i % 100, 24 + i % 100 + 2, 0, 29, 30, 30) for i in range(300)]
    for side in (0, 1):
        got, want = both(al, arena, woff, wlen, recs, 30, side, 75, 24)
        assert np.array_equal(got, want)
        assert np.array_equal(got[14:114], got[114:214]) and (got[14:114] >= 0).all()


def test_window_beyond_two_to_the_31(al):
    """offsets are 64-bit: a window behind byte 2^31 of the arena"""
    import torch
    rng = np.random.default_rng(31)
    w = rand_bases(rng, 150)
    at = (1 << 31) + 101
    arena = torch.empty(at + 150 + 64, dtype=torch.uint8, device="cuda")
    arena[at - 64:] = ord("A")
    arena[at:at + 150] = dev(np.frombuffer(w, dtype=np.uint8))
    small = np.frombuffer(w, dtype=np.uint8)
    off, ln = np.array([at], dtype=np.int64), np.array([150], dtype=np.int32)
    for side, r in ((0, record(10, 39, 0, 29, 30, 30)), (1, record(100, 129, 0, 29, 30, 30))):
        recs = np.array([r], dtype=np.int32)
        got = al.anchor_inserts(arena, dev(off), dev(ln), dev(recs), 30, side).cpu().numpy()
        want = bm.anchor_inserts(small, np.zeros(1, dtype=np.int64), ln, recs, 30, side)
        assert np.array_equal(got, want) and want[0] >= 0


# ---- records of a real scan ----------------------------------------------------------------------------------------------------
def test_records_of_a_real_scan(al, oracle):
    """300 barcoded reads: scan_device's records of both anchors over their windows give the codes the model gives over the
    ORACLE's records of the same pairs"""
    import torch
    planted = bm.make_barcodes(4, 24, 3)
    reads, _ = bm.barcoded_reads(300, planted, 0.08, 3)
    rng = np.random.default_rng(3)
    arena, off, ln = lay_out(rng, [r.encode() for r in reads])
    wl = np.minimum(ln, 150).astype(np.int32)
    offs = [off, off + (ln - wl)]
    n = len(reads)
    d_arena = dev(arena)
    out = torch.empty((2 * n, 8), dtype=torch.int32, device="cuda")
    al.scan_device(d_arena, dev(np.concatenate(offs)), dev(np.concatenate([wl, wl])), np.array([0, 1], dtype=np.int32),
                   np.array([0, n, 2 * n], dtype=np.int64), 150, out)
    anchored = 0
    for side, anchor in enumerate((bm.A_S, bm.A_E)):
        got = al.anchor_inserts(d_arena, dev(offs[side]), dev(wl), out[side * n:(side + 1) * n], len(anchor), side).cpu().numpy()
        recs = np.zeros((n, 8), dtype=np.int32)
        for i, r in enumerate(reads):
            window = r[:150] if side == 0 else r[-150:]
            o = oracle.align_raw(window, anchor, (3, -6, -5, -2))
            recs[i] = [-1, 0, 0, 0, 0, 0, 0, 0] if o.failed else [o.read_start, o.read_end, o.adapter_start, o.adapter_end, o.score,
                                                                   o.aligned_matches, o.aligned_len, o.full_len]
        want = bm.anchor_inserts(arena, offs[side], wl, recs, len(anchor), side)
        assert np.array_equal(got, want)
        anchored += int((want >= 0).sum())
    assert anchored > 300                                              # (f = 0.8 of 600 windows, less what errors unanchor)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(insert_len=0), dict(insert_len=33), dict(side=-1), dict(side=2), dict(min_identity=-1),
                                 dict(min_identity=101), dict(anchor_len=0)])
def test_bad_arguments_are_refused_without_a_launch(al, bad):
    import ctypes
    import torch
    rng = np.random.default_rng(1)
    arena, off, ln = lay_out(rng, [rand_bases(rng, 60)])
    recs = dev(np.array([record(3, 20, 0, 29, 30, 30)], dtype=np.int32))
    codes = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    a = dict(anchor_len=30, side=0, min_identity=75, insert_len=24)
    a.update(bad)
    d_arena, d_off, d_ln = dev(arena), dev(off), dev(ln)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = al.lib.pc_anchor_inserts(al._ctx, d_arena.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), recs.data_ptr(), 1, a["anchor_len"], a["side"],
                                  a["min_identity"], a["insert_len"], codes.data_ptr(), s)
    assert rc == BAD_ARG
    # ... also with n == 0, and before a launch: the output is untouched
    assert al.lib.pc_anchor_inserts(al._ctx, None, None, None, None, 0, a["anchor_len"], a["side"], a["min_identity"], a["insert_len"], None, s) == BAD_ARG
    torch.cuda.synchronize()
    assert int(codes.item()) == -5
    with pytest.raises(RuntimeError, match="bad argument"):
        al.anchor_inserts(d_arena, d_off, d_ln, recs, a["anchor_len"], a["side"], min_identity=a["min_identity"], insert_len=a["insert_len"])
