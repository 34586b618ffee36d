"""The child process of tests/test_gpu_row_classes.py::test_fp16_gate_at_its_column_limit (TEST INFRASTRUCTURE):
    PC_CHECK_RANGE=1 python -m tests.row_class_gate_child <path of the compiled tests/host/plan_probe.cpp>
The library reads PC_CHECK_RANGE once per process: with it the packed-fp16 traced kernel runs its range-checking build, which
records the extremes of every value it forms (pc_debug_value_range) and never traps.  Per scheme of rowclassgen.GATE_SCHEMES
and per row class that pcb::f16_plan admits, two MODE_TRACE calls of 130 windows against an adapter of R bases:

  every window exactly max_cols columns long   records = the oracle's; the range is not (0, 0) and within +-2040: the
                                               packed-fp16 kernel ran, and every value was an exact fp16 integer
  every window max_cols + 1 columns long       records = the oracle's; the range is (0, 0): the packed-int16 kernel ran

max_cols is the probe's (pcb::f16_plan through tests/host/plan_probe.cpp), not re-derived here."""
import sys

import numpy as np
import torch

import porechop_amd
from oracle.oracle import Oracle
from tests import rowclassgen as gen


def main(probe_exe):
    probe = gen.Probe.at(probe_exe)
    oracle = Oracle()
    dev = torch.device("cuda")
    for scheme in gen.GATE_SCHEMES:
        gc = gen.GateCases(probe, scheme)
        al = porechop_amd.Aligner(gc.adapters, scheme)
        al.debug_value_range()
        for rows, at_limit, job in gc.jobs:
            arena = torch.from_numpy(np.frombuffer(job.arena, dtype=np.uint8).copy()).to(dev)
            off = torch.tensor(job.off, dtype=torch.int64, device=dev)
            ln = torch.tensor(job.wlen, dtype=torch.int32, device=dev)
            n = len(job.windows)
            out = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            al.scan_device(arena, off, ln, [job.ad[0]], [0, n], job.max_len, out, gen.MODE_TRACE)
            al.sync()
            lo, hi = al.debug_value_range()
            print("AT_LIMIT" if at_limit else "ABOVE_LIMIT", scheme, "R", rows, "cols", job.max_len, "range", lo, hi, flush=True)
            rec = out.cpu().numpy()
            full = 0
            for i, w in enumerate(job.windows):
                want = oracle.adapter_alignment(w, gc.adapters[job.ad[0]], scheme)
                assert porechop_amd.format_result(rec[i]) == want, (job.name, i, w, porechop_amd.format_result(rec[i]), want)
                full += int(rec[i][4] == scheme[0] * rows)
            assert full >= n // 2, (job.name, full)              # the whole copies were found: M = match R was formed
            if at_limit:
                assert (lo, hi) != (0, 0) and -gen.F16_LIMIT <= lo <= hi <= gen.F16_LIMIT, (job.name, lo, hi)
            else:
                assert (lo, hi) == (0, 0), (job.name, lo, hi)
        al.close()
    print("GATE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
