"""TEST INFRASTRUCTURE, run as a fresh process by tests/test_gpu_wildcards.py with PC_JIT_MIN_CELLS=1 and a private, empty
PC_JIT_CACHE_DIR:  python -m tests.wild_spec_child

The library reads PC_JIT_MIN_CELLS once per process and PC_DISABLE_JIT at every launch, so one process pins both score kernels
in turn for a wildcard context: the generic scan_kernel (PC_DISABLE_JIT=1; pc_jit_stats stays 0, 0) and the specialised kernels,
compiled here for the degenerate pairs.  Whole reads under PC_MODE_TWO_PASS and PC_MODE_SCORE, dual pairs: the degenerate
28-mer | 22-mer, and a pair with 15 and 14 distinct letters per adapter (many letter pairs: the register plan takes its one-wave
form or declines).  Every record is tests/wild_ref.py's, the two kernels' score records are equal byte for byte, and a floored
call at the 90 % floor gives the unfloored records at or above the floor."""
import ctypes
import os
import random
import sys

import numpy as np
import torch

import porechop_amd
from porechop_amd.batch import MODE_SCORE, MODE_TWO_PASS
from tests import wild_ref, wildgen

ADAPTERS = [wildgen.UMI28, wildgen.PRIMER22, "ACGTRYSWKMBDHVNACGTACG", "NVHDBMKWSYRTGCATTGCA"]
SCORES = (3, -6, -5, -2)


def jit_stats():
    compiled, loaded = ctypes.c_int64(0), ctypes.c_int64(0)
    porechop_amd.load_library().pc_jit_stats(ctypes.byref(compiled), ctypes.byref(loaded))
    return compiled.value, loaded.value


def main():
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1" and os.environ.get("PC_JIT_CACHE_DIR") and "PC_DISABLE_JIT" not in os.environ
    assert len(set(ADAPTERS[2].upper())) >= 12 and len(set(ADAPTERS[3].upper())) >= 12
    rng = random.Random(2718)
    reads = []
    for k, (n, where) in enumerate([(n, w) for n in (300, 1100, 3000) for w in ("start", "middle", "end", None) for _ in range(5)]):
        reads.append(wildgen.read_with(rng, n, ADAPTERS[k % 4], where, edits=rng.randrange(0, 3), noise=0.01))
    dev = torch.device("cuda")
    arena = torch.from_numpy(np.frombuffer(("".join(reads) + "N" * 64).encode(), dtype=np.uint8).copy()).to(dev)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    woff, wlen = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    n = len(reads)
    t = (90.0 - 1e-6) / 100.0
    floor = [int(np.floor(len(a) * (t * 3 - 6 * (1.0 - t)))) for a in ADAPTERS]      # pipeline.identity_score_bound at 90 %
    want, cells = {}, {}
    for pair in ((0, 1), (2, 3)):
        c = []
        want[pair], _ = wild_ref.align_many([(r, ADAPTERS[a]) for a in pair for r in reads], SCORES, wildcards=True, cells=c)
        cells[pair] = np.array([[-2, x[0], x[1], 0, w[4], 0, 0, 0] for x, w in zip(c, want[pair])], dtype=np.int32)
    al = porechop_amd.Aligner(ADAPTERS, SCORES, wildcards=True)

    def scan(pair, mode, floors=None):
        out = torch.zeros((2 * n, 8), dtype=torch.int32, device=dev)
        al.scan_device(arena, woff, wlen, [pair[0]], [0, n], int(lens.max()), out, mode, job_adapter_b=[pair[1]],
                       floors=None if floors is None else [floors[0]], floors_b=None if floors is None else [floors[1]])
        al.sync()
        return out.cpu().numpy()

    def all_scans(tag):
        got = {}
        for pair in ((0, 1), (2, 3)):
            traced = scan(pair, MODE_TWO_PASS)
            assert np.array_equal(traced, want[pair]), (tag, pair, np.nonzero((traced != want[pair]).any(axis=1))[0][:5])
            score = scan(pair, MODE_SCORE)
            assert np.array_equal(score, cells[pair]), (tag, pair, np.nonzero((score != cells[pair]).any(axis=1))[0][:5])
            fl = [floor[pair[0]], floor[pair[1]]]
            floored = scan(pair, MODE_TWO_PASS, floors=fl)
            above = np.array([want[pair][k][4] >= fl[k // n] for k in range(2 * n)])
            assert np.array_equal(floored[above], want[pair][above]), (tag, pair)
            assert (floored[~above][:, 0] == -1).all(), (tag, pair)
            got[pair] = (traced, score, floored)
        return got

    os.environ["PC_DISABLE_JIT"] = "1"
    generic = all_scans("generic")
    assert jit_stats() == (0, 0), jit_stats()
    del os.environ["PC_DISABLE_JIT"]
    spec = all_scans("specialised")
    compiled, loaded = jit_stats()
    assert compiled >= 1 and loaded == 0, (compiled, loaded)           # the degenerate 28 | 22 pair has its kernel(s)
    for pair in generic:
        for g, s in zip(generic[pair], spec[pair]):
            assert g.tobytes() == s.tobytes(), pair
    al.close()
    print("wild_spec_child ok compiled=%d" % compiled)


if __name__ == "__main__":
    main()
