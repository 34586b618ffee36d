"""The mask rule of the middle scan's rounds on the GPU (csrc/pc_mask_rule.h, pc_round_select, Pipeline.phase_c) and the
per-call option that keeps the row skip out of the rounds' under-filled launches (pc_scan_device_floored_flags).

One child process (tests/mask_rule_child.py) that pins the specialised score kernels and their row-skipping variants: the
selection kernel against the header's host function; phase_c with the rule against PC_NO_MASK_RULE=1 and against the
reference's sequential logic on the oracle, floored and unfloored, with records that meet a mask by exactly one column; the
row-skip counters of round 0, of the mask rounds and of a mask round that fills the device."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_rounds_scan_only_what_the_mask_can_have_changed_in_a_child_process(tmp_path):
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / "user_cache"))
    for k in ("PC_DISABLE_JIT", "PC_FORCE_CHUNKS", "PC_NO_PASS2_FLOOR", "PC_DISABLE_F16", "PC_NO_ROW_SKIP", "PC_JIT_INT16", "PC_JIT_R0",
              "PC_JIT_CHECK_RANGE", "PC_NO_MASK_RULE", "PC_NO_FUSED_GLUE"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "tests.mask_rule_child"], capture_output=True, text=True, env=env, timeout=600, cwd=REPO)
    assert res.returncode == 0 and "MASK_RULE_CHILD_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
