"""The whole-read score scan's specialised kernel (csrc/pc_jit_source.h) at the edges of its column loop: the 4-column
block, the 16-byte read fetch, the renormalisation of the drifting coordinates, ragged and uniform tiles, one and two
read streams per lane -- PC_MODE_SCORE and PC_MODE_TWO_PASS records against the oracle, field by field.

Each case is one child process (the specialised kernel is forced on from the first launch with PC_JIT_MIN_CELLS=1, which
the library reads once per process) that scans the same windows
  * as one two-adapter job (dual tile: one read stream per lane, rows padded to the longer adapter) and
  * as two single-adapter jobs (two read streams per lane, no padding rows),
with the packed-fp16 kernels, the dual tile again with the packed-int16 ones (pc_set_int16_only), under two scoring schemes:
the default one, and 20/-30/-25/-12, whose fp16 coordinates are renormalised every 208-240 columns -- inside these
reads.  Inputs are seeded and generated here."""
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

la, lb, seed = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
panel = json.load(open("tests/golden/panel.json"))
seqs = []
for s in panel:
    for x in (s["start"], s["end"]):
        if x is not None and x[1] not in seqs:
            seqs.append(x[1])
ad_a = next(q for q in seqs if len(q) == la)
ad_b = next(q for q in seqs if len(q) == lb and q != ad_a)
ads = [ad_a, ad_b]
o = Oracle()


def kren_f16(scores, R):
    """pc_bounds.h spec_plan's period for the packed-fp16 variant (the parent holds it against what the library reports)."""
    match, mismatch, go, ge = scores
    eps = -ge
    low = min(2 * go + (R - 1) * ge, go + (R - 1) * ge + mismatch, go)
    return (2 * 2040 - (match * R - low) - (R + 6) * eps) // eps // 4 * 4


def make_read(rng, n, plants):
    alphabet = rng.choice(["ACGT", "ACGT", "ACGTN", "ACGT-", "acgtACGTUu", "ACGTXN-Uacgt"])
    r = [rng.choice(alphabet) for _ in range(n)]
    for ad, end in plants:                       # a copy of `ad` whose last base is column `end` (1-based), cut at the read's edges
        for k, ch in enumerate(ad):
            c = end - len(ad) + k
            if 0 <= c < n and c < end:
                r[c] = ch
    return "".join(r)


for scores in [(3, -6, -5, -2), (20, -30, -25, -12)]:
    rng = random.Random(seed * 1000 + scores[0])
    R = max(la, lb)
    kren = kren_f16(scores, R)
    print("KREN", scores[0], kren)
    k = kren if kren < 690 else 400              # (default scheme: no renormalisation within 700 columns)
    special = [1, 3, 4, 5, 15, 16, 17, k - 1, k, k + 1, k + 2, 700]
    # columns an adapter copy ends in: 1, either side of a 4-column block edge, of a 16-byte fetch edge and of a renormalisation
    ends = [1, 4, 5, 8, 9, 16, 17, 32, 33, k, k + 1, k + 2, k + 4, k + 5]
    batches = []
    for count in (1, 63, 64, 65, 129):           # ragged tiles: every special length in turn, every third window a random one
        lens, nxt = [], 0
        for i in range(count):
            if i % 3 == 2:
                lens.append(rng.randint(1, 700))
            else:
                lens.append(special[nxt % len(special)])
                nxt += 1
        if count == 1:
            lens = [k + 1]
        else:
            assert set(special) <= set(lens), (count, sorted(set(special) - set(lens)))
        batches.append(lens)
    for count, n in ((64, 17), (65, k + 1), (129, 333), (63, k + 6)):      # every stream of a tile ends in one column
        batches.append([n] * count)
    for bi, lens in enumerate(batches):
        reads = []
        for i, n in enumerate(lens):
            plants = []
            if i % 2 == 0:
                plants.append((ads[(i // 2) % 2], ends[(i // 2) % len(ends)]))
            if i % 5 == 0:
                plants.append((ads[(i // 5) % 2], n))          # ends at the last column
            reads.append(make_read(rng, n, plants))
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
                if not int16:                      # (the two-stream layout with the packed-fp16 kernels only: every kernel is a compile)
                    split = torch.zeros((2 * n, 8), dtype=torch.int32, device="cuda")
                    al.scan_device(arena, woff2, wlen2, [0, 1], [0, n, 2 * n], int(ln.max()), split, mode)
                    al.sync()
                    got[(int16, mode, "split")] = split.cpu().numpy()
        al.close()
        for key, rec in got.items():
            where = (scores, bi, key)
            if key[1] == MODE_SCORE:
                bad = np.nonzero((rec != want_score).any(axis=1))[0]
                assert bad.size == 0, (where, int(bad[0]), lens[int(bad[0]) % n], rec[bad[0]].tolist(), want_score[bad[0]].tolist())
            else:
                for i in range(2 * n):
                    assert porechop_amd.format_result(rec[i]) == want_full[i], (where, i, lens[i % n], rec[i].tolist(), want_full[i])
            assert (rec == got[(False, key[1], "dual")]).all(), where      # layouts and lane types agree record by record
print("SCORE_BLOCK_OK")
'''


@pytest.mark.parametrize("la,lb", [(33, 30), (28, 22), (22, 33), (24, 24)])
def test_score_scan_block_edges_against_the_oracle(la, lb):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_VERBOSE="1")
    res = subprocess.run([sys.executable, "-c", CHILD, str(la), str(lb), "11"], capture_output=True, text=True, env=env,
                         timeout=600, cwd=REPO)
    assert "SCORE_BLOCK_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert "hiprtc" not in res.stderr and "no specialised kernel" not in res.stderr, res.stderr[-2000:]
    # the specialised kernel ran, in both lane types, and the renormalisation period the child planted its edges
    # around is the one the library used for the packed-fp16 kernel of the pair
    R = max(la, lb)
    built = re.findall(r"specialised kernel R=(\d+) K=\d+ f16=(\d) kren=(\d+)", res.stderr)
    assert any(int(r) == R and f == "1" for r, f, _ in built), res.stderr[-2000:]
    assert any(int(r) == R and f == "0" for r, f, _ in built), res.stderr[-2000:]
    krens = {int(k) for r, f, k in built if int(r) == R and f == "1"}
    said = {int(m.group(2)) for m in re.finditer(r"KREN (\d+) (-?\d+)", res.stdout)}
    assert krens <= said and min(krens) < 300, (krens, said)
