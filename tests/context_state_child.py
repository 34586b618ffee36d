"""What tests/test_gpu_context_state.py does to a context (TEST INFRASTRUCTURE): the runner of the script's steps
(tests/stategen.py), and the child process of group G:
    python -m tests.context_state_child
The library reads PC_JIT_MIN_CELLS once per process, so one fresh process started with PC_JIT_MIN_CELLS=1 and a private, empty
PC_JIT_CACHE_DIR runs the specialised score kernels from the first launch on: one context goes P -> Q -> P at the same
adapter indices and then through two schemes, and pc_jit_stats says what the process-wide kernel cache did -- one compile per
distinct (adapter pair, scheme, lane type), none when a list or a scheme returns, nothing from disk."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

from tests import stategen as sg

SENTINEL = np.array(sg.SENTINEL, dtype=np.int32)
FILL = 77                                            # what every output holds before its call: no record has it


class Runner:
    """One context (or several), the material on the device, and what the script expects."""

    def __init__(self, oracle, aligner):
        self.m = sg.material()
        self.expect = sg.Expectations(oracle, self.m)
        self.al = aligner
        self.outs = {}                               # step name -> the records it left on the device
        self._arena, self._windows = {}, {}

    def setup(self, ops, al=None):
        al = al or self.al
        for op in ops:
            arg = self.m.lists[op[1]] if op[0] == "set_adapters" else op[1]
            getattr(al, op[0])(arg)

    def on_device(self, call):
        """-> the arguments of scan_device for this call, up to the output"""
        b = self.m.batch(call.batch)
        if call.batch not in self._arena:
            self._arena[call.batch] = torch.from_numpy(b.arena.copy()).cuda()
        woff, wlen, ja, jb, js, max_len, total = call.arrays(self.m)
        key = (call.batch, len(call.jobs))
        if key not in self._windows:
            self._windows[key] = (torch.from_numpy(woff).cuda(), torch.from_numpy(wlen).cuda())
        d_off, d_len = self._windows[key]
        return self._arena[call.batch], d_off, d_len, ja, js, max_len, jb, total

    def new_out(self, call):
        return torch.full((call.pairs(), 8), FILL, dtype=torch.int32, device="cuda")

    def enqueue(self, call, out, al=None, floors=None):
        arena, d_off, d_len, ja, js, max_len, jb, total = self.on_device(call)
        assert tuple(out.shape) == (total, 8)
        (al or self.al).scan_device(arena, d_off, d_len, ja, js, max_len, out, call.mode, job_adapter_b=jb, floors=floors,
                                    end_rule=call.end_rule, job_side=None if call.sides is None else np.array(call.sides, dtype=np.int32))

    def compare(self, got, want, where):
        """got int32[pairs, 8] from the device against an Expected; -> records that are the no-alignment record"""
        from porechop_amd.batch import format_results
        assert got.shape[0] == len(want.comparable()), where
        if want.score is not None:
            bad = np.nonzero((got != want.score).any(axis=1))[0]
            assert bad.size == 0, (where, "%d of %d score records differ" % (bad.size, got.shape[0]), int(bad[0]), got[bad[0]].tolist(),
                                   want.score[bad[0]].tolist())
            return 0
        have = format_results(got)
        wanted = format_results(want.records) if want.records is not None else want.strings
        gone = (got == SENTINEL).all(axis=1)
        bad = []
        for i, (g, w) in enumerate(zip(have, wanted)):
            if w is None:                                                     # below its floor: the no-alignment record, exactly
                ok = bool(gone[i])
            elif want.may_skip is not None and gone[i]:                       # end rule: only a pair that gives no trim may go
                ok = bool(want.may_skip[i])
            else:
                ok = g == w
            if not ok:
                bad.append(i)
        assert not bad, (where, "%d of %d records differ" % (len(bad), len(have)), bad[:5],
                         [(have[i], wanted[i]) for i in bad[:3]])
        return int(gone.sum())

    def run(self, step):
        """One step of groups A to D on the long-lived context."""
        import pytest
        al, where = self.al, step.where()
        self.setup(step.setup)
        assert (tuple(a.decode() for a in al.adapters), al.scores) == (tuple(step.adapters), tuple(step.scores)), where
        if step.ops_x100 is not None:
            assert al.lib.pc_trace_ops_x100(al._ctx) == step.ops_x100, where
        call = step.call
        out = self.outs[step.source].clone() if step.source else self.new_out(call)
        if step.kind == "enqueue_raises":
            with pytest.raises(RuntimeError):
                self.enqueue(call, out)
            al.sync()
            assert bool((out == FILL).all()), (where, "a refused call wrote records")
            return
        want = self.expect.of(step)
        self.enqueue(call, out, floors=None if want is None or want.floors is None else np.array(want.floors, dtype=np.int32))
        if step.kind == "sync_raises":
            with pytest.raises(RuntimeError):
                al.sync()
            return
        al.sync()
        self.outs[step.name] = out
        gone = self.compare(out.cpu().numpy(), want, where)
        if step.kind == "floored":
            below = sum(s is None for s in want.strings)
            assert gone == below and al.floor_skipped()[0] == below, (where, gone, below, al.floor_skipped())
        elif step.kind == "end_rule":
            # the rule really took pairs out (else the route was not run), and the counter says how many: every skipped
            # pair is a no-alignment record; a window too short for any alignment is one with or without the rule
            skipped = al.floor_skipped()[0]
            assert 0 < skipped == gone < out.shape[0], (where, skipped, gone)


def jit_stats(al):
    c, d = ctypes.c_int64(0), ctypes.c_int64(0)
    al.lib.pc_jit_stats(ctypes.byref(c), ctypes.byref(d))
    return c.value, d.value


def main():
    import porechop_amd
    from oracle.oracle import Oracle
    assert os.environ.get("PC_JIT_MIN_CELLS") == "1" and os.environ.get("PC_JIT_CACHE_DIR") and "PC_DISABLE_JIT" not in os.environ
    m = sg.material()
    al = porechop_amd.Aligner(m.P, sg.DEFAULT)
    r = Runner(Oracle(), al)
    adapters, scores = m.P, sg.DEFAULT
    t0 = time.time()
    try:
        for k, (ops, compiled) in enumerate(sg.child_rounds()):
            r.setup(ops)
            adapters, scores = sg.in_force(m, ops, adapters, scores)
            for call in sg.child_calls():
                where = "G%d %r, mode %d: the process-wide kernel cache (keyed by adapter strings, scheme, lane type)" % (k + 1, ops, call.mode)
                out = r.new_out(call)
                r.enqueue(call, out)
                al.sync()
                r.compare(out.cpu().numpy(), r.expect.of_call(call, adapters, scores), where)
            assert jit_stats(al) == (compiled, 0), (k, ops, jit_stats(al), compiled)
    finally:
        al.close()
    print("CONTEXT_STATE_CHILD_OK %.2f s" % (time.time() - t0))


if __name__ == "__main__":
    sys.exit(main())
