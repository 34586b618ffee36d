"""Compiles pc_bounds.h and pc_cell.h for the HOST and holds the row-skip proposition (pc_bounds.h, row_skip_plan) against the
plain recurrence cell for cell (tests/host/test_row_skip.cpp), under ASan and UBSan: seeded windows of 0-600 columns, the
two headline pairs with their padding and five single adapters, three scoring schemes, floors of 75 / 85 / 90 % and -- on exact copies, where every column of W_low is
needed -- 100 %, every even row the plan accepts.  No GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_skipping_recurrence_against_the_plain_one():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_row_skip")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_row_skip.cpp"), "-o", exe])
        out = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        total = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        assert total["bad"] == 0
        assert total["pairs"] >= 3 * 7 * 3 * 6 * 2
        # the windows are neither always open nor never
        assert 0 < total["columns_on"] < total["columns"]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("scheme ")]
        assert len(lines) == 3
        for ln in lines:
            count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)}
            assert count["plans"] > 0 and count["at_or_above"] > 0 and count["below"] > 0, ln
        # at the default scores the rule finds a row for each of the seven adapter configurations
        assert "rule_rows=7" in lines[0], lines[0]


def test_headline_rows():
    """The rule's rows for the two headline pairs at the default scores: what the shipped kernels are compiled with."""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "r0.cpp")
        exe = os.path.join(tmp, "r0")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "pc_bounds.h"\nint main() { printf("%d %d %d\\n", '
                    'pcb::row_skip_r0(3, -6, -5, -2, 28, 28, 22), pcb::row_skip_r0(3, -6, -5, -2, 33, 33, 30), '
                    'pcb::row_skip_plan(3, -6, -5, -2, 28, 20, 28, 22, 58, 46).w_low); return 0; }\n')
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        # 28 | 22: eight rows skipped, at the floors of 90 % a window of 8 + 26 / 2 = 21 columns; 33 | 30: thirteen rows skipped
        assert out.stdout.split() == ["20", "20", "21"]


def test_the_bounds_header_is_plain_cxx():
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_bounds.h")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text) == ["stdint.h"]
