"""Every kernel on windows behind bytes 2^31 and 2^32 of the arena, and on records behind int 2^31 of the record tensor.

The kernels take int64 offsets (win_off, src_off, dst_off, exc_pos, job_off + r, index[k]) and must carry them in 64 bits
to the load or store; a 32-bit carry is exact in every other test of the suite, whose arenas are a few hundred KB.  Here
ONE small block of windows (tests/fargen.py) sits four times in a 4.3 GB arena that is allocated and never filled -- at
byte 0, across 2^31, across 2^32 and behind 2^32 -- and every kernel family runs one call over all four placements:
  (a) the records or masks of the three far placements equal those of the placement at byte 0, element for element;
  (b) the placement at byte 0 equals the plain reference exactly (the oracle's DP, its edit distance, Python slices,
      tests/glue_ref.py and tests/explain_ref.py).
The record-indexed kernels of phase B run on a record tensor of 2^28 + 2^16 records (8.6 GB, never filled either) with
their jobs' records across record 2^28 = int 2^31, against the same jobs at record 0 and the host references.

At most two of the large buffers are alive at a time (arena 4.3 GB + plane 1.1 GB, or the record tensor alone); the
module skips only where less than 12 GB of device memory is free."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import fargen, glue_ref, gluegen
from tests.fargen import B31, B32, PLACEMENTS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED_FREE = 12 << 30
REC_EDGE = 1 << 28                        # record 2^28 starts at int 2^31 of the record tensor
REC_TOTAL = REC_EDGE + (1 << 16)


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()                  # (a copy: buffers of bytes objects are read-only)


class Far:
    """The far arena and its 2-bit plane, written only where the four placements lie.  ensure(variant) (re)allocates them
    and writes the block ("mixed": every alphabet; "acgt": the same windows made of A/C/G/T); release() frees them."""

    def __init__(self):
        self.dp, self.nine, self.long200, every = fargen.far_adapters()
        self.layout, self.acgt = fargen.make_layout(fargen.SEED, every)
        self.block = self.layout.block
        self.n = self.block.n
        self.max_len = self.block.max_len
        self.arena = self.plane = self.exc = None
        self.variant = None
        self.d_off, self.d_len = dev(self.layout.win_off), dev(self.layout.win_len)
        self._want = {}

    def ensure(self, variant="mixed"):
        import torch
        if self.arena is None:
            self.arena = torch.empty(fargen.ARENA_BYTES, dtype=torch.uint8, device="cuda")
            self.plane = torch.empty(fargen.PLANE_BYTES, dtype=torch.uint8, device="cuda")
            self.variant = None
        if self.variant != variant:
            block = self.block if variant == "mixed" else self.acgt
            packed, exc = self.layout.packed_images(block)
            for name in PLACEMENTS:
                first, data = self.layout.image(name, block)
                self.arena[first:first + len(data)] = dev(np.frombuffer(data, dtype=np.uint8))
                at, pk, _ = packed[name]
                self.plane[at:at + pk.size] = dev(pk)
            self.exc_host = exc
            self.exc = dev(exc)
            self.variant = variant
            torch.cuda.synchronize()
        return self

    def release(self):
        import torch
        self.arena = self.plane = self.exc = None
        self.variant = None
        torch.cuda.empty_cache()

    def by_placement(self, x):
        """[4 n, ...] per-window results -> [4, n, ...]"""
        return x.reshape((len(PLACEMENTS), self.n) + x.shape[1:])

    # ---- the plain references, computed once per (adapter, scheme) -------------------------------------------------------
    def want_full(self, oracle, ad, scores):
        key = ("full", ad, scores)
        if key not in self._want:
            self._want[key] = [oracle.adapter_alignment(r, ad, scores) for r in self.block.reads]
        return self._want[key]

    def want_score(self, oracle, ad, scores):
        key = ("score", ad, scores)
        if key not in self._want:
            rows = []
            for r in self.block.reads:
                x = oracle.align_raw(r, ad, scores)
                rows.append([-2, x.end_j, x.end_i, 0, x.score, 0, 0, 0])
            self._want[key] = np.array(rows, dtype=np.int32)
        return self._want[key]

    def want_edits(self, oracle, ad, variant):
        key = ("edits", ad, variant)
        if key not in self._want:
            block = self.block if variant == "mixed" else self.acgt
            self._want[key] = oracle.min_edits_many(np.frombuffer(block.data, dtype=np.uint8), block.off, block.len, ad)
        return self._want[key]


@pytest.fixture(scope="module")
def far():
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip("less than 12 GB of device memory free (%.1f GB)" % (free / 2**30))
    torch.cuda.reset_peak_memory_stats()
    f = Far()
    yield f
    print("far offsets: max_memory_allocated %.2f GB" % (torch.cuda.max_memory_allocated() / 2**30))
    f.release()
    del f
    torch.cuda.empty_cache()


# ---- DP scans -----------------------------------------------------------------------------------------------------------
def scan_jobs(far, al, jobs, mode, init=None):
    """One pc_scan_device call: every job (adapter, second adapter or -1) over all 4 n windows.  -> per job and adapter
    (adapter index, records [4, n, 8]) and the raw output."""
    import torch
    far.ensure()
    k, nw = len(jobs), 4 * far.n
    woff, wlen = far.d_off.repeat(k), far.d_len.repeat(k)
    total = sum(nw * (2 if b >= 0 else 1) for _, b in jobs)
    out = torch.zeros((total, 8), dtype=torch.int32, device="cuda") if init is None else init.clone()
    al.scan_device(far.arena, woff, wlen, [a for a, _ in jobs], [j * nw for j in range(k + 1)], far.max_len, out, mode,
                   job_adapter_b=[b for _, b in jobs])
    al.sync()
    host, parts, pos = out.cpu().numpy(), [], 0
    for a, b in jobs:
        for x in ((a, b) if b >= 0 else (a,)):
            parts.append((x, far.by_placement(host[pos:pos + nw])))
            pos += nw
    return parts, out


def check_records(far, oracle, ads, scores, parts, score_only, what):
    from porechop_amd.batch import format_results
    for a, rec in parts:
        where = (what, len(ads[a]))
        if score_only:
            want = far.want_score(oracle, ads[a], scores)
            bad = np.nonzero((rec[0] != want).any(axis=1))[0]
            assert bad.size == 0, (where, "near against the oracle", bad[:5].tolist(), rec[0][bad[:3]].tolist(), want[bad[:3]].tolist())
        else:
            got, want = format_results(rec[0]), far.want_full(oracle, ads[a], scores)
            bad = [i for i in range(far.n) if got[i] != want[i]]
            assert not bad, (where, "near against the oracle", bad[:5], [(got[i], want[i]) for i in bad[:3]])
        for k, name in enumerate(PLACEMENTS[1:], 1):
            bad = np.nonzero((rec[k] != rec[0]).any(axis=1))[0]
            assert bad.size == 0, (where, name, "differs from near", bad[:5].tolist(), far.block.len[bad[:5]].tolist(),
                                   rec[k][bad[:3]].tolist(), rec[0][bad[:3]].tolist())


DUAL_AND_SINGLE = [(0, 1), (2, 3), (4, -1), (0, -1)]          # (33 | 30), (28 | 22) as dual jobs; the 24- and the 33-mer alone


@pytest.mark.parametrize("int16", [False, True])
def test_traced_end_window_kernels(far, oracle, int16):
    """PC_MODE_TRACE: single-adapter and dual jobs, the packed-fp16 traced kernel and (set_int16_only) the packed-int16 one."""
    import porechop_amd
    from porechop_amd.batch import MODE_TRACE
    al = porechop_amd.Aligner(far.dp, fargen.SCORES)
    try:
        al.set_int16_only(int16)
        parts, _ = scan_jobs(far, al, DUAL_AND_SINGLE, MODE_TRACE)
        check_records(far, oracle, far.dp, fargen.SCORES, parts, False, ("trace", int16))
    finally:
        al.close()


@pytest.mark.parametrize("int16", [False, True])
def test_trace_at_from_the_score_records(far, oracle, int16):
    """PC_MODE_TRACE_AT over the PC_MODE_SCORE records of the same pairs.  (Which score kernel wrote those is the library's
    choice -- the specialised one wherever the kernel cache holds it; the child process below pins both routes.)"""
    import porechop_amd
    from porechop_amd.batch import MODE_SCORE, MODE_TRACE_AT
    al = porechop_amd.Aligner(far.dp, fargen.SCORES)
    try:
        al.set_int16_only(int16)
        jobs = [(0, -1), (1, -1), (2, -1), (3, -1), (4, -1)]
        parts, out_s = scan_jobs(far, al, jobs, MODE_SCORE)
        check_records(far, oracle, far.dp, fargen.SCORES, parts, True, ("score before trace_at", int16))
        parts, _ = scan_jobs(far, al, jobs, MODE_TRACE_AT, init=out_s)
        check_records(far, oracle, far.dp, fargen.SCORES, parts, False, ("trace_at", int16))
    finally:
        al.close()


def test_linear_gap_scheme_lds_state_kernel(far, oracle):
    """3/-6/-5/-5: gap_open == gap_extend takes the generic kernel with its state in LDS, traced and two-pass."""
    import porechop_amd
    from porechop_amd.batch import MODE_TRACE, MODE_TWO_PASS
    scores = (3, -6, -5, -5)
    al = porechop_amd.Aligner(far.dp, scores)
    try:
        for mode in (MODE_TRACE, MODE_TWO_PASS):
            parts, _ = scan_jobs(far, al, [(0, 1), (2, -1)], mode)
            check_records(far, oracle, far.dp, scores, parts, False, ("linear", mode))
    finally:
        al.close()


@pytest.mark.parametrize("layout", ["lds", "hbm"])
def test_plain_int32_kernel(far, oracle, layout):
    """slow_kernel in both state layouts: 3/-6/-5/0 with a 28-mer (state in LDS) and a 200-base adapter under the default
    scheme (state in HBM)."""
    import porechop_amd
    from porechop_amd.batch import MODE_TRACE
    ads, scores = ([far.dp[2]], (3, -6, -5, 0)) if layout == "lds" else ([far.long200], fargen.SCORES)
    al = porechop_amd.Aligner(ads, scores)
    try:
        parts, _ = scan_jobs(far, al, [(0, -1)], MODE_TRACE)
        check_records(far, oracle, ads, scores, parts, False, ("plain int32", layout))
    finally:
        al.close()


# The score pass by both routes, each pinned, in one child process (the library reads PC_JIT_MIN_CELLS once per process and
# PC_DISABLE_JIT at every launch).  A kernel that is on disk is used from the first launch whatever the batch size, so "a small
# batch" does not select the generic kernels: PC_DISABLE_JIT=1 does, and pc_jit_stats shows that nothing was loaded or built.
SCORE_CHILD = r'''
import ctypes, os, sys
sys.path.insert(0, ".")
import numpy as np, torch
import porechop_amd
from porechop_amd.batch import MODE_SCORE, MODE_TWO_PASS
from oracle.oracle import Oracle
from tests import fargen
from tests.test_gpu_far_offsets import Far, scan_jobs, check_records, DUAL_AND_SINGLE


def jit_stats(al):
    c, d = ctypes.c_int64(), ctypes.c_int64()
    al.lib.pc_jit_stats(ctypes.byref(c), ctypes.byref(d))
    return c.value, d.value


def both_modes(al, what):
    for int16 in (False, True):
        al.set_int16_only(int16)
        for mode in (MODE_SCORE, MODE_TWO_PASS):
            parts, out = scan_jobs(far, al, DUAL_AND_SINGLE, mode)
            check_records(far, o, far.dp, fargen.SCORES, parts, mode == MODE_SCORE, (what, mode, int16))


far, o = Far(), Oracle()
al = porechop_amd.Aligner(far.dp, fargen.SCORES)
os.environ["PC_DISABLE_JIT"] = "1"                   # ---- the generic kernels: scan_kernel's score pass, plan_kernel, the second pass
both_modes(al, "generic")
assert jit_stats(al) == (0, 0), jit_stats(al)        # no specialised kernel was loaded from disk or compiled: none can have run
print("FAR_GENERIC_OK")
del os.environ["PC_DISABLE_JIT"]                     # ---- pc_spec_score, from the first launch
both_modes(al, "specialised")
print("JIT_STATS %d %d" % jit_stats(al))
al.close()
far.release()
print("FAR_SPEC_OK")
'''


def test_generic_and_specialised_score_kernels_in_a_child_process(far, tmp_path):
    """PC_MODE_SCORE and PC_MODE_TWO_PASS, fp16 and int16 lanes, dual and single-adapter jobs: first through the generic
    kernels (PC_DISABLE_JIT=1; pc_jit_stats stays 0, 0) -- plan_kernel's win_off + c0 and the lead-in before a window that
    starts right at 2^32 --, then with pc_spec_score forced (PC_JIT_MIN_CELLS=1).  The packed-fp16 kernels of the four
    panel jobs must come from the cache built with the library: the user cache is a fresh directory.  The parent's buffers
    are freed for the child's arena and come back with the next test."""
    import re
    far.release()
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_VERBOSE="1", PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    env.pop("PC_DISABLE_JIT", None)
    res = subprocess.run([sys.executable, "-c", SCORE_CHILD], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert "FAR_GENERIC_OK" in res.stdout and "FAR_SPEC_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert "hiprtc" not in res.stderr and "no specialised kernel" not in res.stderr, res.stderr[-2000:]
    built = re.findall(r"specialised kernel R=(\d+) K=\d+ f16=(\d) kren=-?\d+ waves/CU=\d+ \(([^)]*)\)", res.stderr)
    f16 = [(int(r), where) for r, f, where in built if f == "1"]
    i16 = [int(r) for r, f, _ in built if f == "0"]
    # (33 | 30), (28 | 22), the 24-mer and the 33-mer alone: four kernels per lane type
    assert sorted(r for r, _ in f16) == [24, 28, 33, 33] and sorted(i16) == [24, 28, 33, 33], res.stderr[-2000:]
    assert all(where == "from the kernel cache on disk" for _, where in f16), res.stderr[-2000:]
    compiled, from_disk = map(int, re.search(r"JIT_STATS (\d+) (\d+)", res.stdout).groups())
    assert compiled + from_disk == 8 and from_disk >= 4, (compiled, from_disk)


# ---- prefilter ----------------------------------------------------------------------------------------------------------
def bits_of(mask, na):
    return ((mask[:, :, None] >> np.arange(32)[None, None, :]) & 1).reshape(mask.shape[0], -1)[:, :na].T.astype(bool)      # [na, 4 n]


def check_mask(far, oracle, mask, ks, variant, exact, what):
    """(b) near against the oracle's edit distance: nothing within the bound cleared (every adapter), and -- where the mask
    is exact -- nothing beyond it kept for adapters of at most 32 bases; (a) the far placements equal near."""
    got = bits_of(mask, len(far.nine))
    lens = far.block.len
    for j, (ad, k) in enumerate(zip(far.nine, ks)):
        rows = far.by_placement(got[j])
        within = (far.want_edits(oracle, ad, variant) <= k) & (lens > 0)
        for p, name in enumerate(PLACEMENTS):                        # soundness everywhere
            missed = np.nonzero(within & ~rows[p])[0]
            assert missed.size == 0, (what, name, "a window within the bound was cleared", len(ad), k, missed[:5].tolist())
        if exact and len(ad) <= 32:
            wrong = np.nonzero(rows[0] != within)[0]
            assert wrong.size == 0, (what, "near against the oracle", len(ad), k, wrong[:5].tolist())
        for p, name in enumerate(PLACEMENTS[1:], 1):
            bad = np.nonzero(rows[p] != rows[0])[0]
            assert bad.size == 0, (what, name, "differs from near", len(ad), k, bad[:5].tolist(), lens[bad[:5]].tolist())
    kept = far.by_placement(got.any(axis=0))[0]
    assert 0 < int(kept.sum()) and int((~got).sum()) > 0


@pytest.fixture(scope="module")
def pf(far):
    import porechop_amd
    al = porechop_amd.Aligner(far.nine)
    yield al
    al.close()


@pytest.mark.parametrize("thr", fargen.THRESHOLDS)
def test_prefilter_byte_route(far, oracle, pf, thr):
    """90 %: seed scan and verification; 85 % and 70 %: pieces the exhaustive kernel takes."""
    far.ensure()
    ks = [pf.max_edits(len(a), thr) for a in far.nine]
    mask = pf.prefilter_mask(far.arena, far.d_off, far.d_len, far.max_len, list(range(9)), ks)
    pf.sync()
    check_mask(far, oracle, mask.cpu().numpy(), ks, "mixed", True, ("bytes", thr))


@pytest.mark.parametrize("thr", fargen.THRESHOLDS)
def test_prefilter_plane_route(far, oracle, pf, thr):
    """win_off in bases.  Where a read holds a letter that is not a base the plane route keeps a superset of the byte
    route's pairs, so the exact comparison with the oracle is made on the A/C/G/T variant below."""
    far.ensure()
    ks = [pf.max_edits(len(a), thr) for a in far.nine]
    mask = pf.prefilter_mask_packed(far.plane, far.d_off, far.d_len, far.max_len, list(range(9)), ks, total=True)
    by = pf.prefilter_mask(far.arena, far.d_off, far.d_len, far.max_len, list(range(9)), ks)
    pf.sync()
    mask, by = mask.cpu().numpy(), by.cpu().numpy()
    check_mask(far, oracle, mask, ks, "mixed", False, ("plane", thr))
    assert np.all((by & ~mask) == 0), thr                           # nothing the byte route keeps is dropped


@pytest.mark.parametrize("thr", fargen.THRESHOLDS)
def test_prefilter_routes_agree_bit_for_bit_on_acgt(far, oracle, pf, thr):
    far.ensure("acgt")
    try:
        ks = [pf.max_edits(len(a), thr) for a in far.nine]
        by = pf.prefilter_mask(far.arena, far.d_off, far.d_len, far.max_len, list(range(9)), ks)
        pl = pf.prefilter_mask_packed(far.plane, far.d_off, far.d_len, far.max_len, list(range(9)), ks, total=True)
        pf.sync()
        by, pl = by.cpu().numpy(), pl.cpu().numpy()
        diff = np.nonzero((by != pl).any(axis=1))[0]
        assert diff.size == 0, (thr, [(PLACEMENTS[i // far.n], i % far.n) for i in diff[:5].tolist()])
        check_mask(far, oracle, pl, ks, "acgt", True, ("plane, acgt", thr))
        check_mask(far, oracle, by, ks, "acgt", True, ("bytes, acgt", thr))
    finally:
        far.ensure("mixed")


# ---- bytes from the plane, copies, trimmed windows ------------------------------------------------------------------------
def canonical(far, i):
    """Window i of the block as pc_unpack_* writes it: A C G T (lower case and U folded), 'N' for everything else."""
    raw = np.frombuffer(far.block.reads[i].encode("latin-1"), dtype=np.uint8)
    table = np.full(256, ord("N"), dtype=np.uint8)
    for src, dst in zip(b"ACGTUacgtu", b"ACGTTACGTT"):
        table[src] = dst
    return table[raw]


def strided_offsets(lens, base):
    stride = (lens.astype(np.int64) + 23) // 16 * 16
    return np.concatenate([[0], np.cumsum(stride)]).astype(np.int64) + base


@pytest.mark.parametrize("dst_base", [1 << 20, B31 + (1 << 20)])
def test_unpack_windows(far, dst_base):
    """Source windows at the four placements (exceptions on both sides of 2^32), written into a slice view of the far
    arena: destination offsets below 2^31 and above it."""
    import porechop_amd
    far.ensure()
    b = far.block
    idx = np.concatenate([np.array(b.disjoint) + k * far.n for k in range(4)])
    src, ln = far.layout.win_off[idx], far.layout.win_len[idx]
    assert np.all(src[1:] >= (src + ln)[:-1])
    view_at = 1 << 19                                            # the view starts half a MB into the arena
    do = strided_offsets(ln, dst_base)
    lo, hi = view_at + int(do[0]), view_at + int(do[-1])
    for name in PLACEMENTS:                                      # the copies land between the placements
        first, data = far.layout.image(name)
        assert hi + 64 <= first or first + len(data) <= lo
    al = porechop_amd.Aligner(["ACGT"])
    try:
        far.arena[lo - 64:hi + 64] = 0xEE
        al.unpack_windows(far.plane, far.exc, dev(src), dev(ln), far.arena[view_at:], dev(do), pad=ord("-"))
        al.sync()
        got = far.arena[lo - 64:hi + 64].cpu().numpy()
    finally:
        al.close()
    assert np.all(got[:64] == 0xEE) and np.all(got[-64:] == 0xEE)
    rel = do - do[0] + 64
    for k, (i, l) in enumerate(zip(idx.tolist(), ln.tolist())):
        want = canonical(far, i % far.n)
        assert np.array_equal(got[rel[k]:rel[k] + l], want), (PLACEMENTS[i // far.n], i % far.n, l)
        assert np.all(got[rel[k] + l:rel[k + 1]] == ord("-")), (PLACEMENTS[i // far.n], i % far.n)


@pytest.mark.parametrize("dst_base", [1 << 20, B31 + (1 << 20)])
def test_copy_windows(far, dst_base):
    """Far sources, far destinations (a slice view of the arena itself, between the placements)."""
    import porechop_amd
    far.ensure()
    src, ln = far.layout.win_off, far.layout.win_len
    view_at = 1 << 19
    do = strided_offsets(ln, dst_base)
    lo, hi = view_at + int(do[0]), view_at + int(do[-1])
    for name in PLACEMENTS:
        first, data = far.layout.image(name)
        assert hi + 64 <= first or first + len(data) <= lo
    al = porechop_amd.Aligner(["ACGT"])
    try:
        far.arena[lo - 64:hi + 64] = 0xEE
        al.copy_windows(far.arena, far.d_off, far.d_len, far.arena[view_at:], dev(do), ord("N"))
        al.sync()
        got = far.arena[lo - 64:hi + 64].cpu().numpy()
    finally:
        al.close()
    assert np.all(got[:64] == 0xEE) and np.all(got[-64:] == 0xEE)
    rel = do - do[0] + 64
    for k, l in enumerate(ln.tolist()):
        want = np.frombuffer(far.block.reads[k % far.n].encode("latin-1"), dtype=np.uint8)
        assert np.array_equal(got[rel[k]:rel[k] + l], want), (PLACEMENTS[k // far.n], k % far.n, l)
        assert np.all(got[rel[k] + l:rel[k + 1]] == ord("N")), (PLACEMENTS[k // far.n], k % far.n)


def test_trim_windows_with_offsets_behind_two_to_the_32(far):
    import porechop_amd
    rng = np.random.default_rng(32)
    off, ln = far.layout.win_off, far.layout.win_len
    n = off.shape[0]
    st = np.tile(np.where(rng.random(far.n) < 0.3, 0, rng.integers(0, 200, size=far.n)), 4).astype(np.int32)
    et = np.tile(np.where(rng.random(far.n) < 0.3, 0, rng.integers(0, 200, size=far.n)), 4).astype(np.int32)
    al = porechop_amd.Aligner(["ACGT"])
    try:
        toff, tlen, stats = al.trim_windows(far.d_off, far.d_len, dev(st), dev(et))
        al.sync()
    finally:
        al.close()
    import torch
    assert toff.dtype == torch.int64 and stats.dtype == torch.int64
    toff, tlen = toff.cpu().numpy(), tlen.cpu().numpy()
    want = [glue_ref.trimmed_interval(int(ln[i]), int(st[i]), int(et[i])) for i in range(n)]
    ws, wl = np.array([w[0] for w in want], dtype=np.int64), np.array([w[1] for w in want], dtype=np.int64)
    assert np.array_equal(tlen, wl) and np.array_equal(toff, off + ws)
    assert (toff >= B32).sum() > far.n and stats.cpu().tolist() == glue_ref.trim_stats(wl.tolist())
    rel, lens = far.by_placement(toff - np.repeat([far.layout.start[p] for p in PLACEMENTS], far.n)), far.by_placement(tlen)
    for k in range(1, 4):
        assert np.array_equal(rel[k], rel[0]) and np.array_equal(lens[k], lens[0]), PLACEMENTS[k]


def test_unpack_device_of_more_than_two_to_the_32_bases(far):
    """pc_unpack_device over the whole plane into the far arena's own storage (then rewritten).  Compared on the host: 4 KB
    around base 0, 2^31 and 2^32, the four images (every exception lies in one), and the tail with its pad."""
    import porechop_amd
    import torch
    far.ensure()
    nbases = B32 + (1 << 20) + 40000 + 7                       # not a multiple of 16: the byte-wise tail
    assert nbases + 64 <= fargen.ARENA_BYTES and far.exc_host.max() < nbases
    spans = [(0, 4096), (B31 - 2048, B31 + 2048), (B32 - 2048, B32 + 2048), (nbases - 4096, nbases + 64)]
    for name in PLACEMENTS:
        first, data = far.layout.image(name)
        spans.append((first, first + len(data)))
    codes = {}
    for lo, hi in spans:                                        # the plane's bytes under each span, before the arena is overwritten
        codes[lo] = far.plane[lo // 4:(min(hi, nbases) + 3) // 4].cpu().numpy()
    al = porechop_amd.Aligner(["ACGT"])
    try:
        far.variant = None                                      # the arena's placements are about to be overwritten
        far.arena[nbases + 64:nbases + 128] = 0xEE
        out = al.unpack_device(far.plane, nbases, far.exc, arena=far.arena, pad=64)
        al.sync()
        assert out.data_ptr() == far.arena.data_ptr()
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        for lo, hi in spans:
            got = far.arena[lo:hi].cpu().numpy()
            p = codes[lo]
            want = letters[((p[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)[None, :]) & 3).reshape(-1)][lo % 4:]
            want = np.concatenate([want[:min(hi, nbases) - lo], np.full(max(0, hi - nbases), ord("N"), dtype=np.uint8)])
            e = far.exc_host[(far.exc_host >= lo) & (far.exc_host < hi)]
            want[e - lo] = ord("N")
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (lo, hi, (bad[:5] + lo).tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        assert bool((far.arena[nbases + 64:nbases + 128] == 0xEE).all())      # nothing behind the pad
        # and the images hold the block's canonical bytes (the plane was packed from them)
        for name in PLACEMENTS:
            s = far.layout.start[name]
            got = far.arena[s:s + len(far.block.data)].cpu().numpy()
            for i in (0, far.block.designated, far.n - 1):
                o, l = int(far.block.off[i]), int(far.block.len[i])
                assert np.array_equal(got[o:o + l], canonical(far, i)), (name, i)
    finally:
        al.close()
        far.ensure("mixed")


# ---- one end-to-end check: the pipeline over reads laid out across 2^32 ---------------------------------------------------
def test_pipeline_over_reads_across_two_to_the_32(far, oracle):
    import torch
    from porechop_amd.pipeline import AdapterSet, DeviceReads, Pipeline, ScanParams
    from tests import ref_pipeline
    from tests.golden_io import load_panel
    from tests.pairgen import mutate, synthetic_read
    rng = random.Random(4032)
    reads = []
    for i in range(200):
        ln = rng.choice([1000, 1500, 2200, 3000])
        r = synthetic_read(rng, ln, fargen.Y_TOP if rng.random() < 0.8 else None, fargen.Y_BOTTOM if rng.random() < 0.6 else None,
                           (fargen.Y_BOTTOM + fargen.Y_TOP) if i % 5 == 0 else None)
        if i % 9 == 0:
            p1 = rng.randint(200, ln - 200)
            r = r[:p1] + mutate(rng, fargen.Y_TOP, 0.04) + r[p1:]
        reads.append(r)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    text = np.frombuffer(("".join(reads)).encode() + b"N" * 64, dtype=np.uint8)
    # read 100 starts below 2^32 and ends above it; half of the reads lie on either side
    base = B32 - int(offs[100]) - int(lens[100]) // 2
    assert base + int(offs[100]) < B32 < base + int(offs[100]) + int(lens[100])
    assert base + text.size < far.layout.image("beyond32")[0] and base > far.layout.image("cross31")[0] + (1 << 20)
    far.ensure()
    far.variant = None                                           # the cross32 placement is overwritten; the next test rewrites it
    far.arena[base:base + text.size] = dev(text)
    sets = [AdapterSet(a["name"], tuple(a["start"]) if a["start"] else None, tuple(a["end"]) if a["end"] else None)
            for a in load_panel()]
    p = ScanParams()
    pl = Pipeline(sets, p)
    try:
        matching = [i for i, s in enumerate(pl.sets) if s.name == "SQK-NSK007"]
        results = []
        for arena, shift in ((far.arena, base), (dev(text), 0)):
            rd = DeviceReads(arena, dev(offs + shift), dev(lens))
            st, et = pl.phase_b(rd, matching)
            row = [st.cpu(), et.cpu()]
            for prove in (False, True):
                hits = pl.phase_c(rd, st, et, matching, prove=prove)
                pl.aligner.sync()
                order = torch.argsort(hits.read * 4096 + hits.start.to(torch.int64), stable=True).cpu()
                row += [t.cpu()[order] for t in (hits.read, hits.adapter, hits.start, hits.end, hits.identity)]
            results.append(row)
        for a, b in zip(*results):
            assert torch.equal(a, b)
        st, et = results[0][0].tolist(), results[0][1].tolist()
        for k in range(5):                                          # the proven scan finds the same hits
            assert torch.equal(results[0][2 + k], results[0][7 + k]), k
        assert results[0][2].numel() >= 40
        got = {}
        for r, a, s, e in zip(*(results[0][k].tolist() for k in (2, 3, 4, 5))):
            got.setdefault(r, set()).add((a, s, e))
        sample = [99, 100, 101] + random.Random(1).sample(range(200), 21)
        for r in sample:
            assert (st[r], et[r]) == ref_pipeline.phase_b(oracle.adapter_alignment, reads[r], pl.sets, matching, p), r
            want = ref_pipeline.phase_c(oracle.adapter_alignment, reads[r], st[r], et[r], pl.middle_adapters, p)
            assert got.get(r, set()) == {(a, s, e) for a, s, e, _ in want}, (r, got.get(r), want)
    finally:
        pl.close()
        far.ensure("mixed")


# ---- record indices beyond 2^31 ints --------------------------------------------------------------------------------------
class Records:
    pass


@pytest.fixture(scope="module")
def big(far):
    """The record tensor of 2^28 + 2^16 records, allocated after the far arena and its plane are freed."""
    import porechop_amd
    import torch
    far.release()
    h = Records()
    h.t = torch.empty((REC_TOTAL, 8), dtype=torch.int32, device="cuda")
    h.al = porechop_amd.Aligner(["ACGTACGTAC"])
    yield h
    h.al.close()
    h.t = None
    torch.cuda.empty_cache()


def far_base(count):
    """First record of a table of `count` records that has record 2^28 in its middle."""
    base = REC_EDGE - count // 2
    assert base > count and base + count <= REC_TOTAL
    return base


def reduce_inputs(n=257, J=9, nbins=4, seed=28):
    from tests.test_gpu_glue_kernels import reduce_case
    rng = np.random.default_rng(seed)
    recs, offs, sides, bins = reduce_case(rng, n, J, nbins)
    return rng, recs, offs, sides, bins


@pytest.mark.parametrize("masked", [False, True])
def test_phase_b_reduce_on_far_records(big, masked):
    import torch
    from tests.test_gpu_glue_kernels import host_reduce
    n, J = 257, 9
    rng, recs, offs, sides, bins = reduce_inputs(n, J)
    base = far_base(len(recs))
    assert (offs + base < REC_EDGE).any() and (offs + base >= REC_EDGE).any()
    big.t[:len(recs)] = dev(recs)
    big.t[base:base + len(recs)] = dev(recs)
    mask = gluegen.traced_mask(rng, J, n) if masked else None
    p, thr, diff = (150, 50, 2, 100.0 / 3), 33.333333, 0.0
    want = host_reduce(recs, offs, sides, bins, n, gluegen.unpack_bits(mask, n) if masked else None, p, thr, diff, False)
    got = []
    for o in (offs, offs + base):
        st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        et = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        call = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        big.al.phase_b_reduce(big.t, n, o, sides, *p, st, et, bins=bins, barcode_threshold=thr, barcode_diff=diff, require_two=False,
                              call=call, traced_mask=None if mask is None else dev(mask))
        big.al.sync()
        got.append((st.cpu().tolist(), et.cpu().tolist(), call.cpu().tolist()))
    assert got[0] == tuple(want), "records at 0 against the host reference"
    assert got[1] == got[0], "records across 2^28 differ from the same records at 0"
    assert len(set(want[0])) > 3 and len(set(want[2])) > 1


@pytest.mark.parametrize("masked", [False, True])
def test_phase_b_explain_on_far_records(big, masked):
    from tests import explain_ref, explaingen
    n, J, nbins = 257, 24, 5
    rng = np.random.default_rng(280 + masked)
    recs, offs, sides, bins = explaingen.case(rng, n, J, nbins, shared_jobs=True)
    offs = np.asarray(offs, dtype=np.int64)
    base = far_base(len(recs))
    assert (offs + base < REC_EDGE).any() and (offs + base >= REC_EDGE).any()
    big.t[:len(recs)] = dev(recs)
    big.t[base:base + len(recs)] = dev(recs)
    mask = gluegen.traced_mask(rng, J, n) if masked else None
    p = (150, 50, 2, 75.0)
    want = explain_ref.explain(recs, n, offs, sides, *p, bins=bins, traced=gluegen.unpack_bits(mask, n) if masked else None)
    got = []
    for o in (offs, offs + base):
        out = big.al.phase_b_explain(big.t, n, o, sides, *p, bins=bins or None, traced_mask=None if mask is None else dev(mask))
        big.al.sync()
        got.append(tuple(t.cpu().numpy() for t in out))
    for name, g0, g1, w in zip(("summary", "bscore", "hit_first", "hits"), got[0], got[1], want):
        assert g0.shape == w.shape and np.array_equal(g0, w), ("records at 0 against the host model", name)
        assert np.array_equal(g1, g0), ("records across 2^28 differ from the same records at 0", name)
    assert want[3].shape[0] > 100


def test_phase_b_select_on_far_records(big):
    """Both rounds, against tests/glue_ref.select_round (the rules of the exact pruning per read, in plain Python) and
    against the same records at record 0."""
    import torch
    n, J, m = 257, 8, 24
    scores = (3, -6, -5, -2)                                        # the scheme of the module's aligner
    rng = np.random.default_rng(2828)
    recs = np.stack([np.full(J * n, -2), rng.integers(0, 151, size=J * n), rng.integers(0, m + 1, size=J * n), np.zeros(J * n, np.int64),
                     rng.integers(-20, 3 * m + 1, size=J * n), np.zeros(J * n, np.int64), np.zeros(J * n, np.int64),
                     np.zeros(J * n, np.int64)], axis=1).astype(np.int32)
    recs[::17] = gluegen.end_records(rng, len(recs[::17]), 150, 50, zeros=False)      # records that are not plain score records
    offs = (rng.permutation(J) * n).astype(np.int64)
    base = far_base(len(recs))
    assert (offs + base < REC_EDGE).any() and (offs + base >= REC_EDGE).any()
    big.t[:len(recs)] = dev(recs)
    big.t[base:base + len(recs)] = dev(recs)
    side = np.array([0, 1, 0, 1, 1, 0, 0, 1], dtype=np.int32)
    jlen = np.array([m, m, 22, 28, m, 33, m, 30], dtype=np.int32)
    calls = (np.arange(J) % 2).astype(np.int32)
    sl = rng.choice([150, 150, 150, 90, 20], size=n).astype(np.int32)
    el = rng.choice([150, 150, 150, 90, 20], size=n).astype(np.int32)
    st = rng.choice([0, 10, 40, 120], size=n).astype(np.int32)
    et = rng.choice([0, 12, 60, 140], size=n).astype(np.int32)
    best0 = np.where(rng.random((2, n)) < 0.5, 0.0, rng.choice([50.0, 75.0, 100.0 * 22 / 24], size=(2, n)))
    words = (n + 63) // 64
    p, level, diff = (150, 4, 2, 75.0), 70.0, 5.0
    got = []
    for o in (offs, offs + base):
        best = dev(best0)
        m1 = torch.zeros((J, words), dtype=torch.int64, device="cuda")
        c1 = torch.zeros(J, dtype=torch.int64, device="cuda")
        ub_t = torch.zeros((J, n), dtype=torch.int32, device="cuda")
        ub_f = torch.zeros((J, n), dtype=torch.float64, device="cuda")
        big.al.phase_b_select(big.t, n, dev(o), dev(side), dev(jlen), dev(calls), dev(sl), dev(el), *p, 1, level, diff, m1, c1,
                              best_full=best, ub_trim_out=ub_t, ub_full_out=ub_f)
        m2 = torch.zeros((J, words), dtype=torch.int64, device="cuda")
        c2 = torch.zeros(J, dtype=torch.int64, device="cuda")
        big.al.phase_b_select(big.t, n, dev(o), dev(side), dev(jlen), dev(calls), dev(sl), dev(el), *p, 2, level, diff, m2, c2,
                              mask_prev=m1, start_trim=dev(st), end_trim=dev(et), best_full=best)
        big.al.sync()
        got.append([t.cpu().numpy() for t in (m1, c1, ub_t, ub_f, m2, c2)])
    # records at 0 against the host model
    args = (recs.tolist(), offs.tolist(), side.tolist(), jlen.tolist(), calls.tolist(), sl.tolist(), el.tolist(), n, p, scores)
    want1, want_t, want_f = glue_ref.select_round(*args, 1, level, diff)
    want2, _, _ = glue_ref.select_round(*args, 2, level, diff, prev=want1, so_far=(st.tolist(), et.tolist()), best_full=best0.tolist())
    bits1, bits2 = gluegen.unpack_bits(got[0][0], n), gluegen.unpack_bits(got[0][4], n)
    assert np.array_equal(got[0][2], np.array(want_t)) and np.array_equal(got[0][3], np.array(want_f)), "bounds at 0 against the host model"
    assert np.array_equal(bits1, np.array(want1)), ("round 1 at 0 against the host model", np.argwhere(bits1 != np.array(want1))[:5].tolist())
    assert np.array_equal(bits2, np.array(want2)), ("round 2 at 0 against the host model", np.argwhere(bits2 != np.array(want2))[:5].tolist())
    assert got[0][1].tolist() == bits1.sum(axis=1).tolist() and got[0][5].tolist() == bits2.sum(axis=1).tolist()
    for name, a, b in zip(("mask 1", "counts 1", "ub_trim", "ub_full", "mask 2", "counts 2"), got[0], got[1]):
        assert np.array_equal(a, b), ("records across 2^28 differ from the same records at 0", name)
    # the case is not degenerate: both rounds select some pairs and leave some, by the trim rule and by the call rule
    assert n < int(bits1.sum()) < J * n - n and n // 4 < int(bits2.sum()) < J * n - int(bits1.sum())
    assert len(set(got[0][2].reshape(-1).tolist())) > 5 and (got[0][2] == 0).any()


def test_gather_records_and_phase_b_gather_behind_record_two_to_the_28(big):
    import torch
    n, J = 257, 6
    rng = np.random.default_rng(2829)
    count = J * (n + 2)
    recs = rng.integers(-2**31, 2**31, size=(count, 8)).astype(np.int32)
    base = far_base(count)
    big.t[:count] = dev(recs)
    big.t[base:base + count] = dev(recs)
    # gather_records: duplicate and unsorted indices on both sides of record 2^28
    idx = rng.integers(0, count, size=1000).astype(np.int64)
    idx[:4] = [count // 2 - 1, count // 2, 0, count - 1]
    near = big.al.gather_records(big.t, dev(idx))
    there = big.al.gather_records(big.t, dev(idx + base))
    big.al.sync()
    assert ((idx + base) < REC_EDGE).any() and ((idx + base) >= REC_EDGE).any()
    assert np.array_equal(near.cpu().numpy(), recs[idx]) and np.array_equal(there.cpu().numpy(), recs[idx])
    # phase_b_gather: job offsets across record 2^28, window offsets behind byte 2^32
    bits = rng.random((J, ((n + 63) // 64) * 64)) < 0.4
    bits[:, n:] = False
    bits[1] = False
    mask = gluegen.pack_bits(bits)
    cnt = bits.sum(axis=1)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    T = int(cnt.sum())
    job_off = (rng.permutation(J) * (n + 2)).astype(np.int64)
    side = rng.integers(0, 2, size=J).astype(np.int32)
    so = rng.integers(B32 - 10**6, B32 + 10**6, size=n).astype(np.int64)
    eo = rng.integers(B32 - 10**6, B32 + 10**6, size=n).astype(np.int64)
    sl = rng.integers(0, 150, size=n).astype(np.int32)
    el = rng.integers(0, 150, size=n).astype(np.int32)
    for shift in (0, base):
        cursor = dev(np.full(J, 12345, dtype=np.int64))
        win_off = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
        win_len = torch.full((T + 1,), -1, dtype=torch.int32, device="cuda")
        dest = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
        pjob = torch.full((T + 1,), -1, dtype=torch.int32, device="cuda")
        pread = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")
        big.al.phase_b_gather(dev(mask), n, dev(first), cursor, dev(job_off + shift), dev(side), dev(so), dev(sl), dev(eo), dev(el),
                              win_off, win_len, dest, pjob, pread)
        big.al.sync()
        assert cursor.cpu().tolist() == cnt.tolist()
        wo, wl, de, pj, pr = (t.cpu().numpy() for t in (win_off, win_len, dest, pjob, pread))
        assert (wo[T], wl[T], de[T], pj[T], pr[T]) == (-1, -1, -1, -1, -1)
        for j in range(J):
            lo, hi = int(first[j]), int(first[j] + cnt[j])
            assert sorted(pr[lo:hi].tolist()) == np.nonzero(bits[j, :n])[0].tolist(), (shift, j)
            assert (pj[lo:hi] == j).all()
            assert np.array_equal(de[lo:hi], job_off[j] + shift + pr[lo:hi]), (shift, j)
            o, L = (eo, el) if side[j] else (so, sl)
            assert np.array_equal(wo[lo:hi], o[pr[lo:hi]]) and np.array_equal(wl[lo:hi], L[pr[lo:hi]]), (shift, j)
        if shift:
            assert (de[:T] < REC_EDGE).any() and (de[:T] >= REC_EDGE).any() and (wo[:T] >= B32).any()
            # the gathered records of those pairs, as the traced scan would take them
            picked = big.al.gather_records(big.t, dest[:T].contiguous())
            big.al.sync()
            assert np.array_equal(picked.cpu().numpy(), recs[de[:T] - shift])


def test_phase_b_scatter_on_far_records(big):
    n, J = 257, 5
    rng = np.random.default_rng(2830)
    records = gluegen.end_records(rng, J * n, 150, 50).reshape(J * n, 8)
    count = (J * n) // 2
    local = rng.choice(J * n, size=count, replace=False).astype(np.int64)
    pjob, pread = (local // n).astype(np.int32), (local % n).astype(np.int64)
    traced = gluegen.end_records(rng, count, 150, 50)
    traced[::3, 5] = traced[::3, 7]
    side = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    calls = np.array([1, 1, 0, 1, 0], dtype=np.int32)
    best0 = np.where(rng.random((2, n)) < 0.3, [glue_ref.identity(2, 3)], 0.0)
    want = records.copy()
    want[local] = traced
    wb = best0.copy()
    F = glue_ref.record_fields(traced)
    for k in range(count):
        j = int(pjob[k])
        if calls[j] and traced[k, 0] != -1 and traced[k, 7] > 0:
            wb[side[j], pread[k]] = max(wb[side[j], pread[k]], F[k][0])
    base = far_base(J * n)
    assert ((local + base) < REC_EDGE).any() and ((local + base) >= REC_EDGE).any()
    for shift in (0, base):
        big.t[shift - 8 if shift else 0:shift + J * n + 8] = 77
        big.t[shift:shift + J * n] = dev(records)
        best = dev(best0)
        big.al.phase_b_scatter(dev(traced), dev(local + shift), dev(pjob), dev(pread), big.t, dev(side), dev(calls), best, n)
        big.al.sync()
        got = big.t[shift:shift + J * n].cpu().numpy()
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (shift, bad[:5].tolist())
        assert bool((big.t[shift + J * n:shift + J * n + 8] == 77).all()) and (shift == 0 or bool((big.t[shift - 8:shift] == 77).all()))
        assert np.array_equal(best.cpu().numpy(), wb), shift
