"""Alignments that REACH the bounds of the two-pass scan (csrc/pc_bounds.h), on every route that relies on one of them.

tests/stretchgen.py builds, with the oracle, adapter copies stretched by runs of filler bases until the path is as wide as
W, the per-pair bound I + (match*I - score)/g and the warm-up SPAN allow (tests/test_stretchgen_cpu.py shows that they
get there), ending 1, 2, span - m - 1, span - 1, span and span + 1 columns behind each chunk boundary, in tiles that also
hold exact copies, reads without a hit, early hits and shorter reads.  Each route runs in a child process of its own
(tests/stretch_child.py: the library reads its switches once per process) under all eight schemes; every record, both
halves of the dual job included, must be the oracle's string, and the kernel that really ran is pinned the way
test_gpu_parity.py does it (pc_trace_ops_x100: 1325 packed fp16, 2100 packed int16; pc_jit_stats for the score pass)."""
import os
import pickle
import re
import subprocess
import sys

import pytest

from tests import stretchgen as sg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PC_NO_PAIR_TRACE_BOUND", "PC_DISABLE_F16", "PC_FORCE_CHUNKS", "PC_DISABLE_JIT", "PC_JIT_MIN_CELLS", "PC_JIT_INT16", "PC_JIT_VERBOSE",
            "PC_NO_END_ORDER", "PC_DEBUG_TRACE", "PC_CHECK_RANGE")
# The traced kernel of a scheme (pc_bounds.h f16_plan for the 28-row class over 150 columns, which is what pc_trace_ops_x100
# reports): packed fp16 where every value stays an exact fp16 integer -- not under the linear schemes (their extension is
# replaced by -12000), not with an extension of 40 or 140 (the drift of 150 columns leaves +-2040).
FP16 = {(3, -6, -5, -2), (3, -6, -2, -5), (5, -4, -10, -1), (20, -30, -25, -12)}
DEFAULT_AT, OTHER_AT = sg.SCHEMES.index(sg.DEFAULT), sg.SCHEMES.index((3, -6, -2, -5))


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    """The batches of every scheme and their oracle strings, computed once and handed to every child as one file."""
    batches = {}
    for sc in sg.SCHEMES:
        batches[sc] = sg.batch(oracle, sc)
        for job in batches[sc]:
            job["tight"] = sg.tight_windows(oracle, sc, job)
    path = tmp_path_factory.mktemp("stretched") / "batches.pickle"
    with open(path, "wb") as f:
        pickle.dump(batches, f)
    return str(path)


def child(route, data, tmp_path, select=(), **switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches, PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    res = subprocess.run([sys.executable, "-m", "tests.stretch_child", route, data, *select], capture_output=True, text=True, env=env,
                         timeout=600, cwd=REPO)
    assert res.returncode == 0 and "STRETCH_OK " + route in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    ops = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"^OPS (\d+) (\d+) ", res.stdout, re.M)}
    jit = tuple(int(x) for x in re.search(r"^JIT (\d+) (\d+)", res.stdout, re.M).groups())
    return ops, jit, res


def expected_ops(int16=False):
    return {i: (1325 if sc in FP16 and not int16 else 2100) for i, sc in enumerate(sg.SCHEMES)}


def test_two_pass_per_pair_trace_bound(data, tmp_path):
    """Route 1, the default of the headline middle scan: packed-fp16 traced kernel, plan_kernel's per-pair trace_cols,
    end-aligned tiles.  (First GPU run: 2.2 s, after 4.1 s once per module for the batches and their oracle strings.)"""
    ops, _, _ = child("two_pass", data, tmp_path)
    assert ops == expected_ops()


def test_two_pass_adapter_wide_trace_bound(data, tmp_path):
    """Route 2: the packed-fp16 traced kernel with the adapter-wide W + 2 (PC_NO_PAIR_TRACE_BOUND=1).  (First GPU run: 2.1 s.)"""
    ops, _, _ = child("two_pass", data, tmp_path, PC_NO_PAIR_TRACE_BOUND="1")
    assert ops == expected_ops()


def test_two_pass_int16_traced_kernel(data, tmp_path):
    """Route 3: scan_kernel and its notrace_upto = n - W - 2 (PC_DISABLE_F16=1).  (First GPU run: 2.1 s.)"""
    ops, _, _ = child("two_pass", data, tmp_path, PC_DISABLE_F16="1")
    assert ops == expected_ops(int16=True)


def test_score_then_trace_at(data, tmp_path):
    """Route 4: PC_MODE_SCORE, then PC_MODE_TRACE_AT on its records -- whole reads, and windows no longer than the span.
    (First GPU run: 2.5 s.)"""
    ops, _, _ = child("trace_at", data, tmp_path)
    assert ops == expected_ops()


def test_chunked_score_pass_generic_kernels(data, tmp_path):
    """Route 5a: the score pass cut into four column chunks, generic score kernels (every chunk starts SPAN columns early in
    scan_kernel's `cut`).  (First GPU run: 2.3 s.)"""
    ops, jit, _ = child("two_pass", data, tmp_path, PC_FORCE_CHUNKS=str(sg.CHUNKS), PC_DISABLE_JIT="1")
    assert ops == expected_ops() and jit == (0, 0)


def test_chunked_score_pass_specialised_kernel_from_the_built_cache(data, tmp_path):
    """Route 5b: pc_spec_score (c0 = start - a.span), the packed-fp16 kernel of (Y_Top | Y_Bottom) under the default scheme
    as the build left it in the kernel cache: nothing is compiled.  (First GPU run: 2.3 s.)"""
    _, jit, res = child("two_pass", data, tmp_path, ["%d:0" % DEFAULT_AT], PC_FORCE_CHUNKS=str(sg.CHUNKS), PC_JIT_MIN_CELLS="1", PC_JIT_VERBOSE="1")
    built = re.findall(r"specialised kernel R=(\d+) K=\d+ f16=(\d) kren=\d+ waves/CU=\d+ \(([^)]*)\)", res.stderr)
    assert jit[0] == 0 and jit[1] >= 1 and built and all(b == ("28", "1", "from the kernel cache on disk") for b in built), (jit, res.stderr[-2000:])


def test_chunked_score_pass_specialised_kernels_compiled_at_run_time(data, tmp_path):
    """Route 5b through hiprtc, four kernels in all: (Y_Top | Y_Bottom) and the 33-mer under (3,-6,-2,-5) in packed fp16, then
    (PC_JIT_INT16=1) the packed-int16 kernels of (Y_Top | Y_Bottom) under the default scheme and under (3,-6,-2,-5).
    (First GPU run: 5.8 s, two children.)"""
    _, jit, res = child("two_pass", data, tmp_path, ["%d:0,1" % OTHER_AT], PC_FORCE_CHUNKS=str(sg.CHUNKS), PC_JIT_MIN_CELLS="1", PC_JIT_VERBOSE="1")
    built = re.findall(r"specialised kernel R=(\d+) K=\d+ f16=(\d)", res.stderr)
    assert jit == (2, 0) and sorted(built) == [("28", "1"), ("33", "1")], (jit, res.stderr[-2000:])
    _, jit, res = child("two_pass", data, tmp_path, ["%d:0" % DEFAULT_AT, "%d:0" % OTHER_AT], PC_FORCE_CHUNKS=str(sg.CHUNKS), PC_JIT_MIN_CELLS="1",
                        PC_JIT_VERBOSE="1", PC_JIT_INT16="1")
    built = re.findall(r"specialised kernel R=(\d+) K=\d+ f16=(\d)", res.stderr)
    assert jit == (2, 0) and built == [("28", "0"), ("28", "0")], (jit, res.stderr[-2000:])
