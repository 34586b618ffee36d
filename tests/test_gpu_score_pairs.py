"""The 2 x 2 blocked column pair of the specialised score kernel (csrc/pc_jit_source.h, column2; packed fp16: 19 ops per
two rows and two columns, U one column ahead) on the GPU: packed fp16 against packed int16 (pc_set_int16_only, which keeps
the six-op recurrence) and both against the oracle, record for record.

Each case is one child process (PC_JIT_MIN_CELLS=1: the specialised kernel from the first launch) and one adapter pair,
scanned as one two-adapter job (tiles of 64 windows, one read stream per lane) and as two single-adapter jobs (tiles of
128 windows, two read streams per lane), PC_MODE_SCORE and PC_MODE_TWO_PASS.  The adapter pairs: R = 1, 2, 3, 4 (no row
pair at all, one pair, a pair and an odd row, two pairs; the library has no specialised kernel for R = 1, that case runs
the generic one), an odd and an even R of the panel, and the headline's (33 | 30) and (28 | 22).

What the window lengths do to the fast path (blocks with j0 > tfmax and j0 + 3 < nmin):
  * PC_MODE_SCORE runs a window in one unit: the fast path is entered at column 1 (the entry conversion of U);
  * PC_MODE_TWO_PASS with PC_FORCE_CHUNKS=4 (set for the child; pc_api.cpp group_chunks_for) cuts every window of the
    two long batches into four column chunks of about 490 columns (the 150-column batch stays whole, the mixed one is
    cut in two): every chunk but the first tracks from column `span` on -- a late tf: one-column path first, then the
    entry conversion -- so a long window enters the fast path four times, once per chunk (within one unit the
    condition is monotone: it is never met again after it failed);
  * ragged tiles: the shortest window of a tile ends the fast path early, the other lanes go on in the one-column path
    (U is used as it stands) and park their last column's state;
  * a tile of windows of PC_KREN + 40 columns (the period of pc_bounds.h spec_plan, about 1 900): the renormalisation
    falls inside the fast stretch; uniform, and ragged by a few columns.
The reads hold a clean copy, a copy with a 6-base insertion, a copy with a 6-base deletion (as far as the adapter has
bases to lose), and copies that end in each of the four columns of a block, so that a new maximum is resolved in each."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, random, sys
sys.path.insert(0, ".")
import numpy as np, torch
import porechop_amd
from porechop_amd.batch import MODE_SCORE, MODE_TWO_PASS
from oracle.oracle import Oracle

ad_a, ad_b = sys.argv[1], sys.argv[2]
if ad_a.isdigit():                               # two lengths: the first adapters of the panel that have them
    la, lb = int(ad_a), int(ad_b)
    seqs = []
    for s in json.load(open("tests/golden/panel.json")):
        for x in (s["start"], s["end"]):
            if x is not None and x[1] not in seqs:
                seqs.append(x[1])
    ad_a = next(q for q in seqs if len(q) == la)
    ad_b = next(q for q in seqs if len(q) == lb and q != ad_a)
ads = [ad_a, ad_b]
scores = (3, -6, -5, -2)
R = max(len(ad_a), len(ad_b))
o = Oracle()
rng = random.Random(1000 + R)

match, mismatch, go, ge = scores
eps = -ge
low = min(2 * go + (R - 1) * ge, go + (R - 1) * ge + mismatch, go)
kren = (2 * 2040 - (match * R - low) - (R + 6) * eps) // eps // 4 * 4      # pc_bounds.h spec_plan, packed fp16
print("KREN", kren)


def variant(ad, kind):
    if kind == 1:                                # 6-base insertion
        c = len(ad) // 2
        return ad[:c] + "".join(rng.choice("ACGT") for _ in range(6)) + ad[c:]
    if kind == 2:                                # 6-base deletion, as far as the adapter has bases to lose
        k = min(6, max(0, len(ad) - 2))
        c = (len(ad) - k) // 2
        return ad[:c] + ad[c + k:]
    return ad


def make_read(i, n):
    r = [rng.choice("ACGT") for _ in range(n)]
    # a copy (clean / insertion / deletion in turn) that ends in column `end` (1-based); the ends walk through the four
    # columns of a block and through the read
    copy = variant(ads[i % 2], (i // 2) % 3)
    end = min(n, len(copy) + 4 * (i % 7) + (i // 8) % 4 + (n // 3 if i % 5 == 0 else 0))
    for k, ch in enumerate(copy):
        c = end - len(copy) + k
        if 0 <= c < n:
            r[c] = ch
    return "".join(r)


long_n = kren + 40
batches = [
    [long_n] * 64,                                                          # the renormalisation inside the fast stretch, uniform end
    [long_n + (i * 5) % 7 for i in range(65)],                              # ... ragged by a few columns; a second tile of one window
    [(1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 21)[i % 13] if i % 3 == 0 else rng.randint(20, 300) for i in range(129)],
    [150] * 128,                                                            # end windows: uniform, two full tiles of 64
]
for bi, lens in enumerate(batches):
    reads = [make_read(i, n) for i, n in enumerate(lens)]
    n = len(reads)
    arena = torch.from_numpy(np.frombuffer("".join(reads).encode() + b"N" * 64, dtype=np.uint8).copy()).cuda()
    ln = np.array(lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.int64)
    woff, wlen = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
    woff2, wlen2 = torch.cat([woff, woff]), torch.cat([wlen, wlen])
    want_score, want_full = [], []
    for ad in ads:
        for r in reads:
            res = o.align_raw(r, ad, scores)
            want_score.append([-2, res.end_j, res.end_i, 0, res.score, 0, 0, 0])
            want_full.append(o.adapter_alignment(r, ad, scores))
    want_score = np.array(want_score, dtype=np.int32)
    got = {}
    al = porechop_amd.Aligner(ads, scores=scores)
    for int16 in (False, True):
        al.set_int16_only(int16)
        for mode in (MODE_SCORE, MODE_TWO_PASS):
            dual = torch.zeros((2 * n, 8), dtype=torch.int32, device="cuda")
            al.scan_device(arena, woff, wlen, [0], [0, n], int(ln.max()), dual, mode, job_adapter_b=[1])
            al.sync()
            got[(int16, mode, "dual")] = dual.cpu().numpy()
            if not int16:
                split = torch.zeros((2 * n, 8), dtype=torch.int32, device="cuda")
                al.scan_device(arena, woff2, wlen2, [0, 1], [0, n, 2 * n], int(ln.max()), split, mode)
                al.sync()
                got[(int16, mode, "split")] = split.cpu().numpy()
    al.close()
    for key, rec in got.items():
        where = (bi, key)
        if key[1] == MODE_SCORE:
            bad = np.nonzero((rec != want_score).any(axis=1))[0]
            assert bad.size == 0, (where, int(bad[0]), lens[int(bad[0]) % n], rec[bad[0]].tolist(), want_score[bad[0]].tolist())
        else:
            for i in range(2 * n):
                assert porechop_amd.format_result(rec[i]) == want_full[i], (where, i, lens[i % n], rec[i].tolist(), want_full[i])
        assert (rec == got[(False, key[1], "dual")]).all(), where          # layouts and lane types agree record by record
    # the copies did end in every column of a block (a new maximum to resolve in each)
    if bi == 3:
        assert {int(j) % 4 for j in want_score[:, 1]} == {0, 1, 2, 3}, sorted({int(j) % 4 for j in want_score[:, 1]})
print("SCORE_PAIRS_OK")
'''


@pytest.mark.parametrize("ad_a,ad_b", [("A", "C"), ("AC", "G"), ("ACG", "TT"), ("ACGT", "GCA"),
                                       ("27", "23"), ("38", "37"), ("33", "30"), ("28", "22")])
def test_blocked_column_pairs_fp16_int16_and_oracle_agree(ad_a, ad_b):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_VERBOSE="1", PC_FORCE_CHUNKS="4")
    res = subprocess.run([sys.executable, "-c", CHILD, ad_a, ad_b], capture_output=True, text=True, env=env,
                         timeout=600, cwd=REPO)
    assert "SCORE_PAIRS_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    R = max(int(ad_a), int(ad_b)) if ad_a.isdigit() else max(len(ad_a), len(ad_b))
    if R < 2:
        return                                   # (pc_jit.cpp: no specialised kernel for one row)
    # (a one-base adapter scanned on its own -- the second job of the two-stream layout -- has none either, and says so)
    said_no = [l for l in res.stderr.splitlines() if "no specialised kernel" in l and "for 1 rows" not in l]
    assert "hiprtc" not in res.stderr and not said_no, res.stderr[-2000:]
    # the specialised kernel ran in both lane types, and the fp16 one with the period the child placed its long windows around
    built = re.findall(r"specialised kernel R=(\d+) K=\d+ f16=(\d) kren=(\d+)", res.stderr)
    assert any(int(r) == R and f == "1" for r, f, _ in built), res.stderr[-2000:]
    assert any(int(r) == R and f == "0" for r, f, _ in built), res.stderr[-2000:]
    said = int(re.search(r"KREN (-?\d+)", res.stdout).group(1))
    assert {int(k) for r, f, k in built if int(r) == R and f == "1"} == {said}, (built, said)
