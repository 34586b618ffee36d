"""The top-aligned layout of the row-skipping score kernels (csrc/pc_bounds.h row_skip_plan_top; csrc/pc_jit_source.h PC_TOP):
the shorter adapter of a pair starts in register row 1 like the longer one, with its padding below it.

tests/row_skip_top_child.py runs twice, each time a child process with a kernel cache of its own: with the default layout
(the shipped kernels of the two headline pairs) and with PC_SKIP_LAYOUT=bottom (the bottom-aligned variants, compiled by the
child).  Each child compares every case's floored call with the same call under PC_NO_ROW_SKIP=1 and with the oracle; here the
two children's records are compared with each other, and the equal-length pair's kernels by the names the cache gives
them (a hash of source and options): for such a pair the layouts are one."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("equal", "uniform", "ragged", "chunks", "halves", "lastcol", "behind", "tiny", "exact", "renorm")


def child(tmp_path, layout):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / ("cache_" + layout)))
    for k in ("PC_DISABLE_JIT", "PC_FORCE_CHUNKS", "PC_NO_PASS2_FLOOR", "PC_DISABLE_F16", "PC_NO_ROW_SKIP", "PC_JIT_INT16", "PC_JIT_R0",
              "PC_JIT_CHECK_RANGE", "PC_SKIP_LAYOUT", "PC_JIT_WAVES"):
        env.pop(k, None)
    if layout == "bottom":
        env["PC_SKIP_LAYOUT"] = "bottom"
    os.makedirs(env["PC_JIT_CACHE_DIR"])
    out = str(tmp_path / (layout + ".npz"))
    res = subprocess.run([sys.executable, "-m", "tests.row_skip_top_child", out], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert res.returncode == 0 and "ROW_SKIP_TOP_CHILD_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    kernels = [ln for ln in res.stdout.splitlines() if ln.startswith("EQUAL_KERNELS ")]
    assert len(kernels) == 1
    return np.load(out), kernels[0].split()[1:], res.stdout


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("row_skip_top")
    return child(tmp, "top"), child(tmp, "bottom")


def test_both_layouts_against_the_plain_scan_and_the_oracle(runs):
    (top, _, top_out), (bottom, _, _) = runs
    print(top_out)
    assert sorted(top.files) == sorted(CASES) and sorted(bottom.files) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_layouts_give_the_same_records(runs, case):
    (top, _, _), (bottom, _, _) = runs
    assert top[case].shape == bottom[case].shape and top[case].shape[1] <= 256
    assert (top[case] == bottom[case]).all()


def test_an_equal_length_pair_has_one_kernel_whatever_the_layout(runs):
    (_, top_kernels, _), (_, bottom_kernels, _) = runs
    # the pair's kernel and its row-skipping variant, and the same two files under both settings
    assert len(top_kernels) == 2 and top_kernels == bottom_kernels, (top_kernels, bottom_kernels)
