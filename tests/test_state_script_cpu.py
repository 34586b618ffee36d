"""The conditions that keep the script of tests/test_gpu_context_state.py (tests/stategen.py) from passing over stale
state, checked on the oracle without a GPU: a context that kept the adapter codes, the scheme or the table of the call
before would give that call's records again -- so every change of state must change the expected records, no step may
expect the same thing whatever the library does, and every piece of state must have its step."""
import numpy as np
import pytest
import torch

from tests import stategen as sg


@pytest.fixture(scope="module")
def expect(oracle):
    return sg.Expectations(oracle)


def differing(a, b):
    a, b = a.comparable(), b.comparable()
    assert len(a) == len(b) and a
    return sum(x != y for x, y in zip(a, b)) / len(a)


def test_every_transition_changes_at_least_a_quarter_of_the_records(expect):
    steps = sg.script()
    pairs = sg.transitions(steps)
    # A: P -> Q, Q -> L, L (and X) -> P, P -> Q under the dual table; B: five changes of scheme under three calls, less the
    # score call the refused scheme does not make and the one behind it, which is held against the scheme before
    assert sum(1 for s, _ in pairs if s.group == "A") == 4 and sum(1 for s, _ in pairs if s.group == "B") == 14
    lowest = 1.0
    for s, t in pairs:
        frac = differing(expect.of(s), expect.of(t))
        lowest = min(lowest, frac)
        assert frac >= 0.25, (s.where(), "against", t.name, frac)
    print("lowest share of records a transition changes: %.3f" % lowest)
    # every setter of adapters or scores in A and B stands before a step that is held against an earlier one, or changes the job list too
    held = {s.name for s, _ in pairs}
    for s in steps:
        if s.group in "AB" and s.kind == "records" and any(op[0] in ("set_adapters", "set_scores") for op in s.setup):
            earlier = [t for t in steps[:steps.index(s)] if t.group == s.group and t.call == s.call]
            assert s.name in held or not earlier, s.where()


def test_the_hit_path_runs_over_other_windows(expect):
    a = [s for s in sg.script() if s.group == "A"]
    assert a[0].call.job_list(sg.material()) == a[1].call.job_list(sg.material()) and a[0].call.batch != a[1].call.batch
    assert (a[0].adapters, a[0].scores) == (a[1].adapters, a[1].scores)
    assert differing(expect.of(a[0]), expect.of(a[1])) >= 0.25           # (a call that answered from the call before would show)


def test_no_degenerate_step(expect):
    steps = sg.script()
    floored = [s for s in steps if s.kind == "floored"]
    ruled = [s for s in steps if s.kind == "end_rule"]
    assert len(floored) == 1 and len(ruled) == 1
    e = expect.of(floored[0])
    skipped = sum(s is None for s in e.strings) / len(e.strings)
    assert 0.25 <= skipped <= 0.75, skipped
    assert len(e.floors) == len(floored[0].call.jobs)
    e = expect.of(ruled[0])
    n = sg.material().batch(ruled[0].call.batch).n
    for k, side in enumerate(ruled[0].call.sides):                       # on either side: pairs that may go and pairs that must stay
        seg = e.may_skip[k * n:(k + 1) * n]
        assert seg.any() and not seg.all(), (k, side)
    assert set(ruled[0].call.sides) == {0, 1}
    # the steps behind them are held to the oracle in full, on the same job list
    i = steps.index(ruled[0])
    assert [s.kind for s in steps[i + 1:i + 3]] == ["records", "records"] and steps[i + 1].call.jobs == floored[0].call.jobs
    assert steps[i + 1].call.mode == sg.MODE_TWO_PASS and steps[i + 2].call.mode == sg.MODE_TRACE
    # the refused calls stand in front of a good one
    for s in steps:
        if s.kind in ("enqueue_raises", "sync_raises"):
            nxt = steps[steps.index(s) + 1]
            assert nxt.group == s.group and nxt.kind == "records", s.where()


def test_switch_steps_expect_unchanged_records_and_both_kernels():
    c = [s for s in sg.script() if s.group == "C"]
    assert {s.ops_x100 for s in c} == {None, sg.OPS_FP16, sg.OPS_INT16}
    reads = [s.ops_x100 for s in c if s.ops_x100 is not None]
    assert reads[:2] == [sg.OPS_FP16, sg.OPS_INT16] and sg.OPS_INT16 == 2100 and sg.OPS_FP16 == 1325
    assert all((s.adapters, s.scores) == (c[0].adapters, c[0].scores) for s in c)
    hints = [op[1] for s in c for op in s.setup if op[0] == "set_length_hint"]
    assert {0, 100, 10000} <= set(hints)
    # every switch is thrown between two identical calls: the table cache hits
    for prev, s in zip(c, c[1:]):
        if any(op[0] in ("set_int16_only", "set_length_hint") for op in s.setup):
            assert prev.call == s.call, s.where()


def test_coverage_on_paper():
    m = sg.material()
    steps = sg.script()
    groups = {s.group for s in steps}
    e = sg.in_flight_calls()
    if e:
        groups.add("E")
    if sg.two_context_rounds() and len(set(sg.TWO_CONTEXT_SCHEMES)) == 2:
        groups.add("F")
    if sg.child_rounds() and sg.child_calls():
        groups.add("G")
    assert sorted(groups) == list(sg.GROUPS)
    lists = [c.job_list(m) for c in e]
    for k, jl in enumerate(lists):
        assert jl not in lists[max(0, k - 2):k], k
    assert [sg.batch_shape(c.batch)[0] for c in e] == [1, 64, 65, 5000, 70000, 3]
    assert max(c.pairs(m) for c in list(e) + [s.call for s in steps]) == 70000          # nothing larger than that batch
    assert len(sg.REDUCES) == 4 and len({(r[1], r[2]) for r in sg.REDUCES}) == 4
    # A: the lists the issue names, in their order; B: its schemes in order, each under three modes
    named = [op[1] for s in steps if s.group == "A" for op in s.setup if op[0] == "set_adapters"]
    assert named == ["P", "Q", "L", "X", "P", "Q", "W", "ONE"]
    assert [len(x) for x in m.P] == [len(x) for x in m.Q] == [22, 24, 28, 33] and set(m.P).isdisjoint(m.Q)
    assert [len(x) for x in m.L] == [6, 40, 63, 111] and len(m.X[4]) == 130 and len(m.W) == 64 and {len(x) for x in m.W} == {24}
    b = [s for s in steps if s.group == "B"]
    assert tuple([op[1] for op in s.setup if op[0] == "set_scores"][-1] for s in b[::3]) == sg.SCHEME_ORDER and not any(s.setup for s in b if s not in b[::3])
    assert [s.call.mode for s in b] == [sg.MODE_TRACE, sg.MODE_SCORE, sg.MODE_TWO_PASS] * len(sg.SCHEME_ORDER)
    d = [s.call.mode for s in steps if s.group == "D"]
    assert {sg.MODE_TRACE, sg.MODE_SCORE, sg.MODE_TRACE_AT, sg.MODE_TWO_PASS, sg.MODE_AUTO} == set(d)
    w = m.batch("w512a")
    assert w.n == 512 and set(w.lens.tolist()) == set(sg.WINDOW_LENS) and m.batch("long64").lens.tolist() == [600] * 64
    # G: P -> Q -> P compiles for P and Q once each and nothing when P returns; a second scheme compiles again
    assert [c for _, c in sg.child_rounds()] == [2, 4, 4, 6, 6]
    nsteps, ncalls, npairs = sg.summary()
    print("script: %d steps, %d scan calls, %d pairs" % (nsteps, ncalls, npairs))


def test_the_stand_in_answers_like_a_new_one_after_set_scores(oracle):
    from tests.cpu_aligner import OracleAligner
    m = sg.material()
    call = sg.Call("b65", sg.DUAL[0], sg.DUAL[1])
    woff, wlen, ja, jb, js, max_len, total = call.arrays(m)
    arena = torch.from_numpy(m.batch("b65").arena.copy())

    def scan(al, mode):
        out = torch.zeros((total, 8), dtype=torch.int32)
        al.scan_device(arena, torch.from_numpy(woff), torch.from_numpy(wlen), ja, js, max_len, out, mode, job_adapter_b=jb)
        return out.numpy()

    live = OracleAligner(oracle, sg.DEFAULT)
    live.set_adapters(m.P)
    first = scan(live, sg.MODE_TRACE)
    live.set_scores(sg.STEEP)
    assert live.scores == sg.STEEP
    new = OracleAligner(oracle, sg.STEEP)
    new.set_adapters(m.P)
    for mode in (sg.MODE_TRACE, sg.MODE_SCORE):
        assert np.array_equal(scan(live, mode), scan(new, mode))
    assert (scan(live, sg.MODE_TRACE) != first).any()
    live.set_scores(list(sg.DEFAULT))
    assert np.array_equal(scan(live, sg.MODE_TRACE), first)
