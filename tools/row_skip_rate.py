#!/usr/bin/env python3
"""The row skip's on-fraction for a leg of tools/run_leg.py: every floored scan call of the leg's steps is followed by a read
of the context's debug counters (pc_set_row_skip_debug / pc_row_skip_blocks: 4-column blocks the row-skipping launches' fast
path ran, and those among them that computed the rows below r0), one line per call.  The reads synchronise: the step
times this prints are not the leg's.
usage: row_skip_rate.py headline|configs4|... [steps]"""
import os
import runpy
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import porechop_amd.batch as batch  # noqa: E402

calls = [0]
total = [0, 0]
plain = batch.Aligner.scan_device


def counted(self, arena, win_off, win_len, job_adapter, job_start, max_len, out, *args, **kw):
    self.set_row_skip_debug(True)
    r = plain(self, arena, win_off, win_len, job_adapter, job_start, max_len, out, *args, **kw)
    if kw.get("floors") is not None or kw.get("floors_b") is not None:
        blocks, on = self.row_skip_blocks(kw.get("stream"))
        calls[0] += 1
        total[0] += blocks
        total[1] += on
        print("floored call %d: %d jobs, %d windows, max_len %d: blocks %d, lower rows on in %d = %.4f %%" % (
            calls[0], len(job_adapter), int(win_off.shape[0]), int(max_len), blocks, on, 100.0 * on / max(1, blocks)))
    return r


batch.Aligner.scan_device = counted
sys.argv = [os.path.join(HERE, "run_leg.py")] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
finally:
    print("ROW_SKIP_RATE calls %d blocks %d on %d = %.4f %%" % (calls[0], total[0], total[1], 100.0 * total[1] / max(1, total[0])))
