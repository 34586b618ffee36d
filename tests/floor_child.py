"""The scan-level checks of tests/test_gpu_pass2_floor.py, run as a child process (TEST INFRASTRUCTURE):
    python -m tests.floor_child
The library reads PC_JIT_MIN_CELLS once per process and PC_DISABLE_JIT at every launch, so one fresh process started with
PC_JIT_MIN_CELLS=1 can pin both score kernels in turn: the generic one (PC_DISABLE_JIT=1; pc_jit_stats stays 0, 0) and the
specialised one.  For each of them, with packed-fp16 and packed-int16 lanes, over a uniform and a ragged batch:

  every pair of a call with floors against the same call without --
    a pair the oracle's score puts below its floor has the record (-1, 0, 0, 0, 0, 0, 0, 0), any other pair the identical record;
    the skipped-pairs counter equals the number of such records;
    with the floors of Pipeline.identity_score_bound no skipped pair is a hit in the unfloored call (the proof, exhaustively);
  the layouts: one pair left in lane 63 of the first tile (every other tile empty), every pair kept (INT32_MIN + 1), none kept
  (INT32_MAX), and the score pass cut into three column chunks (PC_FORCE_CHUNKS=3)."""
import ctypes
import os
import sys

import numpy as np
import torch

import porechop_amd
from oracle.oracle import Oracle
from porechop_amd.batch import MODE_TWO_PASS
from tests import floorgen

SENTINEL = np.array([-1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)


def jit_stats(al):
    c, d = ctypes.c_int64(0), ctypes.c_int64(0)
    al.lib.pc_jit_stats(ctypes.byref(c), ctypes.byref(d))
    return c.value, d.value


def scan(al, b, dev, floors=None, hint=0):
    """The two dual jobs (33 | 30) and (28 | 22) over the batch's reads -> records [4, n, 8] (adapter order of b.ads)."""
    arena, off, ln = dev
    n = floorgen.N_READS
    out = torch.full((4 * n, 8), 77, dtype=torch.int32, device="cuda")
    kw = {}
    if floors is not None:
        kw = dict(floors=[floors[0], floors[2]], floors_b=[floors[1], floors[3]])
    al.set_length_hint(hint)
    al.scan_device(arena, torch.cat([off, off]), torch.cat([ln, ln]), np.array([0, 2], dtype=np.int32), np.array([0, n, 2 * n], dtype=np.int64),
                   b.max_len, out, MODE_TWO_PASS, job_adapter_b=np.array([1, 3], dtype=np.int32), **kw)
    al.sync()
    return out.cpu().numpy().reshape(4, n, 8)


def check(al, b, dev, base, floors, what, hint=0):
    got = scan(al, b, dev, floors, hint)
    below = b.below(floors)
    assert (got[below] == SENTINEL).all(), (what, "a pair below its floor kept a record")
    assert (got[~below] == base[~below]).all(), (what, "a pair at or above its floor changed")
    assert al.floor_skipped()[0] == int(below.sum()), (what, al.floor_skipped(), int(below.sum()))
    return below


def run(al, b, dev, what):
    hint = b.typ_len if b.lens.min() != b.lens.max() else 0
    base = scan(al, b, dev, None, hint)
    assert (base[:, :, 0] != -1).all() and (base[:, :, 4] == b.score).all(), (what, "the unfloored call against the oracle's scores")
    total0 = al.floor_skipped()[1]
    # 1. the floors phase_c hands down: exhaustive proof + equality
    below = check(al, b, dev, base, b.bounds, (what, "bounds"), hint)
    full = np.round(100.0 * base[:, :, 5] / np.maximum(base[:, :, 7], 1), 6)
    assert (full[below] < b.threshold).all(), (what, "a skipped pair is a hit")
    assert (full >= b.threshold).sum() >= 20 and 0 < below.sum() < below.size
    for a, s, want in b.exact:                                  # score == bound is traced, bound - 1 is not
        assert below[a, s] == (want < b.bounds[a]), (what, a, s, want)
    # 2. the layouts
    one = check(al, b, dev, base, floorgen.lane63_floors(b), (what, "lane 63"), hint)
    assert one.sum() == one.size - 1 and not one[0, 63]         # (so three of adapter 0's four tiles hold skipped pairs only)
    assert check(al, b, dev, base, [-2 ** 31 + 1] * 4, (what, "all kept"), hint).sum() == 0
    assert check(al, b, dev, base, [2 ** 31 - 1] * 4, (what, "none kept"), hint).all()
    assert al.floor_skipped()[1] - total0 == int(below.sum()) + one.size - 1 + one.size
    if b.max_len >= 3 * 128:
        os.environ["PC_FORCE_CHUNKS"] = "3"
        try:
            check(al, b, dev, base, b.bounds, (what, "three chunks"), hint)
        finally:
            del os.environ["PC_FORCE_CHUNKS"]
    # an unfloored call through the floored entry point (every floor INT32_MIN) is the unfloored call
    assert (scan(al, b, dev, [floorgen.NO_FLOOR] * 4, hint) == base).all()


def main():
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1"
    o = Oracle()
    batches = [("uniform", floorgen.Batch(o, 11, False)), ("ragged", floorgen.Batch(o, 12, True))]
    al = porechop_amd.Aligner([a[1] for a in batches[0][1].ads], floorgen.SCORES)
    devs = [(torch.from_numpy(b.arena).cuda(), torch.from_numpy(b.offs).cuda(), torch.from_numpy(b.lens).cuda()) for _, b in batches]
    for kernel in ("generic", "specialised"):
        if kernel == "generic":
            os.environ["PC_DISABLE_JIT"] = "1"
        else:
            os.environ.pop("PC_DISABLE_JIT", None)
        for int16 in (False, True):
            al.set_int16_only(int16)
            for (name, b), dev in zip(batches, devs):
                run(al, b, dev, (kernel, "int16" if int16 else "fp16", name))
        if kernel == "generic":
            assert jit_stats(al) == (0, 0), jit_stats(al)       # no specialised kernel can have run
            print("FLOOR_GENERIC_OK")
        else:
            st = jit_stats(al)
            assert st[0] + st[1] >= 4, st                       # (33 | 30) and (28 | 22), both lane types
            print("FLOOR_SPEC_OK")
    al.close()


if __name__ == "__main__":
    sys.exit(main())
