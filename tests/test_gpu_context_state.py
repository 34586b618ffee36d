"""One long-lived scan context through every change of its state (pc_ctx, csrc/pc_api.cpp), as the pipeline, discovery, the
drop-in and the runner use it -- every other GPU test of the scan makes an Aligner, gives it one adapter list and one scheme
and makes a few calls.  The script and its expectations are tests/stategen.py's (the oracle's, never a fresh Aligner's);
tests/test_state_script_cpu.py shows that stale state cannot pass it.  Groups A to F run in this order on ONE module-scoped
Aligner that is never recreated; G is a child process of its own (specialised kernels forced on).  A failing assertion names
the step and the piece of state it was aimed at ("What a context carries from call to call").

  A  the cached tile table: hits over other windows, other adapter lists under the same job list, a refused job list
  B  pc_set_scores on a live context (the lazy panel upload), five changes of scheme under three modes
  C  the switches read at launch time (int16_only, len_hint) under a table cache hit
  D  every mode in turn on one job list; floors and the end rule leave nothing behind; the error word is cleared
  E  six scans and four reductions in flight behind each other: scratch regrown under them, table and reduce slots turning
  F  two contexts in one process, the same adapter strings under two schemes
  G  the process-wide cache of specialised kernels"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import stategen as sg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runner(oracle):
    import porechop_amd
    from tests.context_state_child import Runner
    al = porechop_amd.Aligner(sg.material().P, sg.DEFAULT)
    r = Runner(oracle, al)
    r.context = al._ctx.value
    yield r
    al.close()


def run_group(runner, group):
    t0 = time.time()
    steps = [s for s in sg.script() if s.group == group]
    assert steps
    for step in steps:
        runner.run(step)
        assert runner.al._ctx.value == runner.context                     # the one context, never recreated
    print("group %s: %d steps, %.2f s" % (group, len(steps), time.time() - t0))


def test_a_table_cache_follows_the_adapter_list(runner):
    run_group(runner, "A")


def test_b_scores_change_on_a_live_context(runner):
    run_group(runner, "B")


def test_c_switches_are_read_under_a_cache_hit(runner):
    run_group(runner, "C")


def test_d_modes_in_turn_leave_nothing_behind(runner):
    run_group(runner, "D")


def test_e_calls_in_flight_behind_each_other(runner):
    """No sync between six scans of six job lists over 1, 64, 65, 5 000, 70 000 and 3 windows, each into its own output, and
    four reductions with four job / bin tables: the scratch buffers regrow under the earlier calls' kernels, the table slots
    turn three times and the reduce slots twice.  One sync, then everything against the oracle (the reductions against
    tests/glue_ref.py); then the scans in reverse order."""
    t0 = time.time()
    al, m = runner.al, runner.m
    runner.setup(sg.RESET)
    calls = sg.in_flight_calls()
    want = [runner.expect.of_call(c, m.P, sg.DEFAULT) for c in calls]
    reduces = sg.reduce_cases()
    t1 = time.time()
    outs = [runner.new_out(c) for c in calls]
    for c in calls:
        runner.on_device(c)                                               # (uploads: before anything is in flight)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    red = []
    for recs, offs, sides, bins, n, p, thr, diff, two, _ in reduces:
        red.append((dev(recs), [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]))
    torch.cuda.synchronize()
    for c, out in zip(calls, outs):
        runner.enqueue(c, out)
    for (recs, offs, sides, bins, n, p, thr, diff, two, _), (d_recs, (st, et, call)) in zip(reduces, red):
        al.phase_b_reduce(d_recs, n, offs, sides, *p, st, et, bins=bins, barcode_threshold=thr, barcode_diff=diff, require_two=two, call=call)
    al.sync()
    for k, (c, out, w) in enumerate(zip(calls, outs, want)):
        where = "E scan %d of 6 in flight (%s, %d jobs, mode %d): stream-ordered scratch, the two table slots" % (k + 1, c.batch, len(c.jobs), c.mode)
        assert runner.compare(out.cpu().numpy(), w, where) == 0, where
    for k, ((recs, offs, sides, bins, n, p, thr, diff, two, host), (_, tensors)) in enumerate(zip(reduces, red)):
        for name, t, w in zip(("start_trim", "end_trim", "call"), tensors, host):
            g = t.cpu().tolist()
            bad = [i for i in range(n) if g[i] != w[i]]
            assert not bad, ("E reduction %d of 4 in flight: the two red_slots" % (k + 1), name, bad[:5], [(g[i], w[i]) for i in bad[:5]])
    for out in outs:
        out.fill_(77)
    for c, out in reversed(list(zip(calls, outs))):
        runner.enqueue(c, out)
    al.sync()
    for k, (c, out, w) in enumerate(zip(calls, outs, want)):
        where = "E scan %d of 6, reverse order (%s): scratch that shrinks in use, the slots again" % (k + 1, c.batch)
        assert runner.compare(out.cpu().numpy(), w, where) == 0, where
    assert al._ctx.value == runner.context
    print("group E: expectations %.2f s, device part %.2f s" % (t1 - t0, time.time() - t1))


def test_f_two_contexts_share_nothing_but_the_process(runner):
    """The same adapter strings under two schemes in two contexts, called alternately three times each: the interning, memo
    and kernel tables of the process are keyed by the scheme too."""
    import porechop_amd
    t0 = time.time()
    m = runner.m
    runner.setup(sg.RESET)
    other = porechop_amd.Aligner(m.P, sg.TWO_CONTEXT_SCHEMES[1])
    try:
        for k, call in enumerate(sg.two_context_rounds()):
            for al, scores in zip((runner.al, other), sg.TWO_CONTEXT_SCHEMES):
                out = runner.new_out(call)
                runner.enqueue(call, out, al=al)
                al.sync()
                where = "F round %d, scheme %r: state shared by all contexts of a process" % (k + 1, scores)
                assert runner.compare(out.cpu().numpy(), runner.expect.of_call(call, m.P, scores), where) == 0, where
    finally:
        other.close()
    call = sg.two_context_rounds()[0]                                      # the first context outlives the second
    out = runner.new_out(call)
    runner.enqueue(call, out)
    runner.al.sync()
    runner.compare(out.cpu().numpy(), runner.expect.of_call(call, m.P, sg.DEFAULT), "F: the first context after the second was destroyed")
    # the third context of the process: the default one behind the per-call symbol, whose scheme changes between calls
    # and whose answers are remembered (the second round is answered from the memo, which is keyed by the scheme too)
    b = m.batch("w512a")
    some = [int(np.nonzero(b.lens == ln)[0][k]) for ln in sg.WINDOW_LENS for k in (0, 1)]
    for rnd in (1, 2):
        for i in some:
            for scores in sg.TWO_CONTEXT_SCHEMES:
                for ad in m.P[1:3]:
                    got = porechop_amd.adapter_alignment(b.window(i).decode(), ad, list(scores))
                    want = runner.expect.traced(ad, scores, "w512a")[i]
                    assert got == want, ("F round %d: the default context's scheme, the memo and the interning table" % rnd, i, scores, got, want)
    print("group F: %.2f s" % (time.time() - t0))


def test_g_specialised_kernels_follow_the_adapter_strings(tmp_path):
    t0 = time.time()
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    for k in ("PC_DISABLE_JIT", "PC_FORCE_CHUNKS", "PC_JIT_INT16", "PC_DISABLE_F16"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "tests.context_state_child"], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert res.returncode == 0 and "CONTEXT_STATE_CHILD_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    print("group G: %.2f s (%s)" % (time.time() - t0, res.stdout.strip().splitlines()[-1]))
