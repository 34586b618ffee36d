"""The script of tests/test_gpu_context_state.py (TEST INFRASTRUCTURE; host only, seeded): ONE long-lived scan context taken
through every change of the state it carries from call to call (pc_ctx, csrc/pc_api.cpp) -- other adapter lists and scoring
schemes under an unchanged job list, the switches that are read at launch time, every mode in turn, calls in flight behind
each other, a second context and the process-wide kernel cache.

Material (Material), the steps (script(), in_flight_calls(), reduce_cases(), two_context_rounds(), child_rounds()) and what
every step must return (Expectations).  The expectation of a step is worked out here from the adapters and the scheme the
SCRIPT says are in force, by the oracle (oracle/pc_oracle.c) -- never by another Aligner, which is the code under test:
  traced records   the oracle's 7-field strings (the bulk call's records for the 70 000-window batch), compared through
                   format_result as tests/test_gpu_parity.py does;
  score records    (-2, end_j, end_i, 0, score, 0, 0, 0) from the oracle's align_raw;
  floored calls    the no-alignment record exactly where the oracle's score is below the job's floor;
  end-rule calls   the oracle's record, or the no-alignment record where the oracle's record gives no trim.
tests/test_state_script_cpu.py holds the script to the conditions that keep it from passing over stale state."""
import functools
import random
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

from porechop_amd.batch import MODE_AUTO, MODE_SCORE, MODE_TRACE, MODE_TRACE_AT, MODE_TWO_PASS
from tests.pairgen import mutate

SEED = 20261020
DEFAULT = (3, -6, -5, -2)
STEEP = (20, -30, -25, -12)          # packed kernels; the fp16 coordinates are renormalised inside a 600-base window
LINEAR = (3, -6, -5, -5)             # gap_open == gap_extend: the reference's linear-gap dispatch
REFUSED = (3, -6, 5, -2)             # outside the packed kernels' range: the plain-int32 kernel, no MODE_SCORE
LDS_STATE = (4, -7, -10, -140)       # gap extension too steep to drift: the LDS-state kernel
SCHEME_ORDER = (DEFAULT, STEEP, LINEAR, REFUSED, LDS_STATE, DEFAULT)
END_RULE = (150, 4, 2, 75.0)         # end_size, min_trim_size, extra_end_trim, end_threshold: the reference's defaults
SENTINEL = (-1, 0, 0, 0, 0, 0, 0, 0)
WINDOW_LENS = (1, 7, 40, 90, 149, 150)
BULK_FROM = 20000                    # batches of this many windows take the oracle's bulk call
POOL = 64                            # mutated copies per adapter the windows draw from
OPS_FP16, OPS_INT16 = 1325, 2100     # pc_trace_ops_x100: the packed-fp16 / packed-int16 traced kernel of the 28-row class
GROUPS = "ABCDEFG"
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _seq(rng, m):
    return "".join(rng.choice("ACGT") for _ in range(m))


class Batch:
    """n windows back to back in one arena (64 bytes of 'N' behind the last base)."""

    def __init__(self, name, arena, lens):
        self.name = name
        self.arena = arena
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        self.offs = np.concatenate([[0], np.cumsum(self.lens[:-1], dtype=np.int64)]).astype(np.int64)
        self.n = int(self.lens.shape[0])
        self.max_len = int(self.lens.max())

    def window(self, i):
        o = int(self.offs[i])
        return self.arena[o:o + int(self.lens[i])].tobytes()


#            name       windows  lengths
BATCHES = {"w512a": (512, WINDOW_LENS), "w512b": (512, WINDOW_LENS), "b1": (1, WINDOW_LENS), "b3": (3, WINDOW_LENS),
           "b64": (64, WINDOW_LENS), "b65": (65, WINDOW_LENS), "b5000": (5000, WINDOW_LENS), "b70000": (70000, (150,)),
           "long64": (64, (600,))}


def batch_shape(name):
    """-> (windows, longest window) of a batch, without building it"""
    n, choice = BATCHES[name]
    return n, max(choice[-n:] if n < len(choice) else choice)


class Material:
    """Adapter lists P, Q (the same lengths, other sequences), L (other row classes), X (P and a 130-base adapter: the
    plain-int32 kernel for that adapter alone), W (64 24-mers), ONE (a list of one); the window batches, built on demand.
    Every window carries one copy (0..15 % edits) of an adapter of P and one of an adapter of Q, at random positions, cut at
    the window's end."""

    def __init__(self, seed=SEED):
        rng = random.Random(seed)
        self.seed = seed
        self.P = tuple(_seq(rng, m) for m in (22, 24, 28, 33))
        self.Q = tuple(_seq(rng, m) for m in (22, 24, 28, 33))
        self.L = tuple(_seq(rng, m) for m in (6, 40, 63, 111))
        self.X = self.P + (_seq(rng, 130),)
        self.W = tuple(_seq(rng, 24) for _ in range(64))
        self.ONE = (_seq(rng, 28),)
        self.lists = {"P": self.P, "Q": self.Q, "L": self.L, "X": self.X, "W": self.W, "ONE": self.ONE}
        rates = (0.0, 0.05, 0.10, 0.15)
        self._pools = [[np.frombuffer(mutate(rng, ad, rates[k % 4]).encode(), dtype=np.uint8) for ad in ads for k in range(POOL)]
                       for ads in (self.P, self.Q)]
        self._batches = {}

    def batch(self, name):
        b = self._batches.get(name)
        if b is None:
            n, choice = BATCHES[name]
            b = self._batches[name] = self._make(name, n, choice, self.seed + 1 + sorted(BATCHES).index(name))
        return b

    def _make(self, name, n, choice, seed):
        g = np.random.default_rng(seed)
        if n < len(choice):
            lens = np.array(choice[-n:], dtype=np.int32)                    # (the one-window batch: 150 bases)
        else:
            lens = np.array([choice[i % len(choice)] for i in range(n)], dtype=np.int32)
            g.shuffle(lens)
        offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)])
        arena = np.concatenate([_BASES[g.integers(0, 4, int(lens.sum()))], np.full(64, ord("N"), dtype=np.uint8)])
        at = g.random((n, 2))
        pick = g.integers(0, 4 * POOL, (n, 2))
        for i in range(n):
            ln, o = int(lens[i]), int(offs[i])
            for k in (0, 1):
                pos = int(at[i, k] * ln)
                piece = self._pools[k][pick[i, k]][:ln - pos]
                arena[o + pos:o + pos + piece.shape[0]] = piece
        return Batch(name, arena, lens)


@functools.lru_cache(maxsize=2)
def material(seed=SEED):
    return Material(seed)


@dataclass(frozen=True)
class Call:
    """One scan_device call: job k is adapter jobs[k] (and, in the same tile, jobs_b[k] unless that is -1) over ALL windows
    of the batch -- the windows' offsets are repeated once per job, as tests/test_gpu_score_block.py does."""
    batch: str
    jobs: tuple
    jobs_b: tuple = None
    mode: int = MODE_TRACE
    floors: bool = False                 # MODE_TWO_PASS with a floor per job: the job's median oracle score
    end_rule: tuple = None               # with sides: scan_device(end_rule=..., job_side=...)
    sides: tuple = None

    def segments(self):
        """adapter index of every run of n records in the output: job order, adapter A's records before adapter B's"""
        out = []
        for k, a in enumerate(self.jobs):
            out.append(a)
            if self.jobs_b is not None and self.jobs_b[k] >= 0:
                out.append(self.jobs_b[k])
        return out

    def job_list(self, m):
        """what build_tiles' cache is keyed on (besides mode and end rule)"""
        n, max_len = batch_shape(self.batch)
        return (self.jobs, self.jobs_b, tuple(k * n for k in range(len(self.jobs) + 1)), max_len)

    def pairs(self, m=None):
        return len(self.segments()) * batch_shape(self.batch)[0]

    def arrays(self, m):
        """-> (win_off int64, win_len int32, job_adapter, job_adapter_b or None, job_start, max_len, records in the output)"""
        b = m.batch(self.batch)
        k = len(self.jobs)
        return (np.tile(b.offs, k), np.tile(b.lens, k), np.array(self.jobs, dtype=np.int32),
                None if self.jobs_b is None else np.array(self.jobs_b, dtype=np.int32),
                np.arange(k + 1, dtype=np.int64) * b.n, b.max_len, self.pairs(m))


SINGLE = (0, 1, 2, 3)                    # one job per adapter
DUAL = ((0, 2), (1, 3))                  # the same pairs as two dual jobs: (0 | 1) and (2 | 3)


@dataclass
class Step:
    group: str
    name: str
    state: str                           # the piece of context state the step is aimed at
    setup: tuple                         # Aligner methods called before the scan: (("set_adapters", "Q"), ("set_scores", (..)), ...)
    call: Call
    kind: str                            # records | score | trace_at | floored | end_rule | enqueue_raises | sync_raises
    adapters: tuple                      # the adapter list and the scheme in force, by the script's own book-keeping
    scores: tuple
    source: str = None                   # trace_at, sync_raises: the step whose device records go in as the end cells
    ops_x100: int = None                 # what pc_trace_ops_x100 must read after the setup

    def where(self):
        return "step %s (%s): %s" % (self.name, self.kind, self.state)


def in_force(m, setup, adapters, scores):
    """-> (adapters, scores) in force once `setup` has run: the script's own book-keeping, no question to the context"""
    for op in setup:
        if op[0] == "set_adapters":
            adapters = m.lists[op[1]]
        elif op[0] == "set_scores":
            scores = tuple(op[1])
    return adapters, scores


class _Builder:
    def __init__(self, m):
        self.m, self.steps, self.adapters, self.scores = m, [], m.P, DEFAULT

    def add(self, group, state, call, kind="records", setup=(), **kw):
        self.adapters, self.scores = in_force(self.m, setup, self.adapters, self.scores)
        name = "%s%d" % (group, 1 + sum(1 for s in self.steps if s.group == group))
        self.steps.append(Step(group, name, state, tuple(setup), call, kind, self.adapters, self.scores, **kw))
        return name


RESET = (("set_adapters", "P"), ("set_scores", DEFAULT), ("set_int16_only", False), ("set_length_hint", 0))


@functools.lru_cache(maxsize=2)
def script(seed=SEED):
    """-> the steps of groups A to D, in order (E, F and G: in_flight_calls, two_context_rounds, child_rounds)"""
    m = material(seed)
    b = _Builder(m)
    single = Call("w512a", SINGLE)
    other = Call("w512b", SINGLE)
    dual = Call("w512a", DUAL[0], DUAL[1])
    # ---- A: the cached tile table
    b.add("A", "tile table: built for this job list", single, setup=RESET)
    b.add("A", "tile table: reused (same job list) over other windows of the same count", other)
    b.add("A", "tile table: reused again, the first windows", single)
    b.add("A", "panel upload: other codes under the same lengths and row classes (d_ad_codes, tiles_uploaded)", single,
          setup=(("set_adapters", "Q"),))
    b.add("A", "panel upload: other lengths and row classes under the same job list (d_ad_len, ad_window, ad_span)", single,
          setup=(("set_adapters", "L"),))
    b.add("A", "panel upload: an adapter of the plain-int32 kernel joins (ad_slow, d_slow_ad)", Call("w512a", SINGLE + (4,)),
          setup=(("set_adapters", "X"),))
    b.add("A", "panel upload: back to the first list, nothing of the slow adapter left", single, setup=(("set_adapters", "P"),))
    b.add("A", "tile table: dual jobs (another job list, the other slot)", dual)
    b.add("A", "panel upload under the dual table", dual, setup=(("set_adapters", "Q"),))
    wide = Call("w512b", (0, 7, 13, 21, 34, 47, 55, 63))
    b.add("A", "panel upload: a list of 64 (the tables grow)", wide, setup=(("set_adapters", "W"),))
    one = Call("w512a", (0,))
    b.add("A", "panel upload: a list of one (the tables shrink)", one, setup=(("set_adapters", "ONE"),))
    b.add("A", "tile table: a job list that is refused (adapter index = number of adapters)", Call("w512a", (1,)), kind="enqueue_raises")
    b.add("A", "tile table: the last good call after the refused one (fast path on the table it left)", one)
    # ---- B: scores on a live context, the same three calls under every scheme
    long_single = Call("long64", SINGLE, mode=MODE_TWO_PASS)
    for k, sc in enumerate(SCHEME_ORDER):
        setup = (RESET if k == 0 else ()) + (("set_scores", sc),)
        what = "panel_dirty: scheme %d,%d,%d,%d taken up at the next call" % sc
        b.add("B", what + " (traced)", single, setup=setup)
        b.add("B", what + " (score records)", Call("w512a", SINGLE, mode=MODE_SCORE), kind="enqueue_raises" if sc == REFUSED else "score")
        b.add("B", what + " (two passes, 600-base windows)", long_single)
    # ---- C: switches that are read at launch time, under a table cache hit
    b.add("C", "tile table built; packed-fp16 traced kernel", single, setup=RESET, ops_x100=OPS_FP16)
    b.add("C", "int16_only on under a cached table", single, setup=(("set_int16_only", True),), ops_x100=OPS_INT16)
    b.add("C", "int16_only off under a cached table", single, setup=(("set_int16_only", False),), ops_x100=OPS_FP16)
    b.add("C", "two-pass table built", long_single)
    for hint in (100, 10000, 0):
        b.add("C", "len_hint %d under a cached two-pass table" % hint, long_single, setup=(("set_length_hint", hint),))
    b.add("C", "int16_only on and len_hint 100 under a cached two-pass table", long_single,
          setup=(("set_int16_only", True), ("set_length_hint", 100)), ops_x100=OPS_INT16)
    b.add("C", "both switches back", long_single, setup=(("set_int16_only", False), ("set_length_hint", 0)), ops_x100=OPS_FP16)
    # ---- D: every mode in turn on one job list
    b.add("D", "mode is part of the table's key: traced", single, setup=RESET)
    score = b.add("D", "score records", Call("w512a", SINGLE, mode=MODE_SCORE), kind="score")
    b.add("D", "trace at the end cells of the score records", Call("w512a", SINGLE, mode=MODE_TRACE_AT), kind="trace_at", source=score)
    two = Call("w512a", SINGLE, mode=MODE_TWO_PASS)
    b.add("D", "two passes", two)
    b.add("D", "floors: kBelowFloor marks, d_perm, the bucket counters and the floor counter", Call("w512a", SINGLE, mode=MODE_TWO_PASS, floors=True),
          kind="floored")
    b.add("D", "end rule: the same route by another test (last_end_rule is part of the key)",
          Call("w512a", SINGLE, mode=MODE_AUTO, end_rule=END_RULE, sides=(0, 0, 1, 1)), kind="end_rule")
    b.add("D", "two passes again: no mark, permutation or counter of the floored calls left", two)
    traced = b.add("D", "traced again", single)
    b.add("D", "trace at records that are no score records: the error word", Call("w512a", SINGLE, mode=MODE_TRACE_AT), kind="sync_raises",
          source=traced)
    b.add("D", "a good call after the refused one: the error word is cleared", single)
    return tuple(b.steps)


def in_flight_calls():
    """E: six scans with six job lists (each differs from the two before it) over batches that grow and shrink, enqueued
    without a sync between them: the scratch regrows under the earlier ones, the table slots turn three times."""
    return (Call("b1", SINGLE),
            Call("b64", DUAL[0], DUAL[1], mode=MODE_TWO_PASS),
            Call("b65", (3, 1), mode=MODE_SCORE),
            Call("b5000", (2, 1), (0, -1)),
            Call("b70000", (0,)),
            Call("b3", (1, 2, 3), mode=MODE_TWO_PASS))


#          reads jobs bins  (end_size, min_trim_size, extra_end_trim, end_threshold)  barcode threshold, diff, require two
REDUCES = ((257, 3, 1, (150, 50, 0, 75.0), 75.0, 5.0, False),
           (64, 7, 2, (150, 51, 7, 66.666667), 0.0, 0.0, True),
           (300, 24, 2, (150, 50, 3, 100.0 / 3), 33.333333, 0.0, False),
           (65, 12, 5, (150, 50, 0, 0.0), 66.666667, 100.0 / 3 - 33.333333, True))


def reduce_cases(seed=SEED):
    """E: four phase_b_reduce calls with four job / bin tables (the two red_slots turn twice), each with the trims and calls
    tests/glue_ref.py gives, computed as tests/test_gpu_glue_kernels.py computes them.
    -> [(recs, offs, sides, bins, n, params, threshold, diff, require_two, (start_trim, end_trim, call))]"""
    from tests.test_gpu_glue_kernels import host_reduce, reduce_case
    rng = np.random.default_rng(seed)
    out = []
    for n, J, nbins, p, thr, diff, two in REDUCES:
        recs, offs, sides, bins = reduce_case(rng, n, J, nbins)
        out.append((recs, offs, sides, bins, n, p, thr, diff, two, host_reduce(recs, offs, sides, bins, n, None, p, thr, diff, two)))
    return out


TWO_CONTEXT_SCHEMES = (DEFAULT, STEEP)


def two_context_rounds():
    """F: the calls two contexts with the same adapter strings (P) and two schemes make alternately"""
    return (Call("w512a", SINGLE), Call("w512b", SINGLE, mode=MODE_SCORE), Call("long64", DUAL[0], DUAL[1], mode=MODE_TWO_PASS))


def child_rounds():
    """G (one child process, specialised kernels forced on): (setup, kernels compiled since the process began) per round;
    every round makes child_calls().  Two dual jobs = two adapter pairs, one kernel per (pair, scheme, lane type)."""
    return (((("set_adapters", "P"),), 2), ((("set_adapters", "Q"),), 4), ((("set_adapters", "P"),), 4),
            ((("set_scores", STEEP),), 6), ((("set_scores", DEFAULT),), 6))


def child_calls():
    return (Call("long64", DUAL[0], DUAL[1], mode=MODE_SCORE), Call("long64", DUAL[0], DUAL[1], mode=MODE_TWO_PASS))


@dataclass
class Expected:
    strings: list = None                 # traced: one 7-field string per record; None where the no-alignment record must stand
    records: np.ndarray = None           # traced, bulk batches: the oracle's records (compared through format_results)
    score: np.ndarray = None             # score records, int32 [pairs, 8]
    floors: tuple = None                 # floored: the floor of every job
    may_skip: np.ndarray = None          # end rule: the pairs whose oracle record gives no trim

    def comparable(self):
        if self.score is not None:
            return [tuple(r) for r in self.score.tolist()]
        if self.records is not None:
            return [tuple(r) for r in self.records.tolist()]
        return list(self.strings)


def trim_of(string, side, rule=END_RULE):
    """The trim one traced record would contribute by itself, by the rule of porechop/nanopore_read.py:166-208 as
    tests/end_floor_child.py trims_of_records states it (0: none)."""
    end_size, min_trim_size, extra_end_trim, end_threshold = rule
    f = string.split(",")
    rs, re = int(f[0]), int(f[1]) + 1
    if rs == -1 or not float(f[5]) > end_threshold or re - rs < min_trim_size:
        return 0
    if side == 0:
        return max(0, re + extra_end_trim) if re != end_size else 0
    return max(0, end_size - rs + extra_end_trim) if rs != 0 else 0


class Expectations:
    """What the oracle says a call returns under the adapters and the scheme the script says are in force; every
    (adapter sequence, scheme, batch) is aligned once."""

    def __init__(self, oracle, m=None):
        self.oracle, self.m = oracle, m or material()
        self._traced, self._scored = {}, {}

    def traced(self, adapter, scores, batch):
        key = (adapter, tuple(scores), batch)
        hit = self._traced.get(key)
        if hit is None:
            b = self.m.batch(batch)
            if b.n >= BULK_FROM:
                ad = np.frombuffer(adapter.encode() + b"N", dtype=np.uint8)
                # (the bulk call takes each pair by itself and ctypes drops the interpreter lock: eight slices side by side)
                cuts = [b.n * k // 8 for k in range(9)]
                with ThreadPoolExecutor(8) as pool:
                    r9 = np.concatenate(list(pool.map(
                        lambda k: self.oracle.align_many(b.arena, b.offs[cuts[k]:cuts[k + 1]], b.lens[cuts[k]:cuts[k + 1]], ad,
                                                         np.zeros(cuts[k + 1] - cuts[k], dtype=np.int64),
                                                         np.full(cuts[k + 1] - cuts[k], len(adapter), dtype=np.int32), scores), range(8))))
                hit = np.ascontiguousarray(np.concatenate([r9[:, :7], r9[:, 8:9]], axis=1), dtype=np.int32)
            else:
                hit = [self.oracle.adapter_alignment(b.window(i), adapter, scores) for i in range(b.n)]
            self._traced[key] = hit
        return hit

    def scored(self, adapter, scores, batch):
        key = (adapter, tuple(scores), batch)
        hit = self._scored.get(key)
        if hit is None:
            b = self.m.batch(batch)
            rows = []
            for i in range(b.n):
                r = self.oracle.align_raw(b.window(i), adapter, scores)
                rows.append((-2, r.end_j, r.end_i, 0, r.score, 0, 0, 0))
            hit = self._scored[key] = np.array(rows, dtype=np.int32).reshape(-1, 8)
        return hit

    def of_call(self, call, adapters, scores, kind=None):
        kind = kind or ("score" if call.mode == MODE_SCORE else "records")
        seg = call.segments()
        if kind == "score":
            return Expected(score=np.concatenate([self.scored(adapters[a], scores, call.batch) for a in seg]))
        parts = [self.traced(adapters[a], scores, call.batch) for a in seg]
        if isinstance(parts[0], np.ndarray):
            return Expected(records=np.concatenate(parts))
        strings = [s for p in parts for s in p]
        if kind == "floored":
            assert call.jobs_b is None
            n = self.m.batch(call.batch).n
            best = np.array([int(s.split(",")[4]) for s in strings]).reshape(len(seg), n)
            floors = tuple(int(np.sort(row)[n // 2]) for row in best)
            below = (best < np.array(floors)[:, None]).reshape(-1)
            return Expected(strings=[None if lo else s for s, lo in zip(strings, below)], floors=floors)
        if kind == "end_rule":
            assert call.jobs_b is None
            n = self.m.batch(call.batch).n
            no_trim = np.array([trim_of(s, call.sides[k // n], call.end_rule) == 0 for k, s in enumerate(strings)])
            return Expected(strings=strings, may_skip=no_trim)
        return Expected(strings=strings)

    def of(self, step):
        if step.kind in ("enqueue_raises", "sync_raises"):
            return None
        return self.of_call(step.call, step.adapters, step.scores, "records" if step.kind == "trace_at" else step.kind)


def transitions(steps):
    """(step, the latest earlier step of its group that made the identical call) for every step whose adapter sequences or
    scheme differ from that earlier step's: the steps that pass over stale state unless their records differ."""
    out = []
    for i, s in enumerate(steps):
        if s.kind not in ("records", "score"):
            continue
        for t in reversed(steps[:i]):
            if t.group == s.group and t.call == s.call and t.kind == s.kind:
                used = lambda st: tuple(st.adapters[a] for a in st.call.segments())
                if used(t) != used(s) or t.scores != s.scores:
                    out.append((s, t))
                break
    return out


def summary(seed=SEED):
    """-> (steps, scan calls, (window, adapter) pairs) of the whole script, the second run of E's scans and G included"""
    m = material(seed)
    steps = script(seed)
    calls = [s.call for s in steps] + list(in_flight_calls()) * 2 + list(two_context_rounds()) * 2
    calls += list(child_calls()) * len(child_rounds())
    nsteps = len(steps) + 2 * len(in_flight_calls()) + len(REDUCES) + 2 * len(two_context_rounds()) + len(child_rounds())
    return nsteps, len(calls), sum(c.pairs(m) for c in calls)
