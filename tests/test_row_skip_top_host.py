"""Compiles pc_bounds.h and pc_cell.h for the HOST and holds the row-skip proposition of the TOP-aligned layout (pc_bounds.h,
row_skip_plan_top) against the plain recurrence cell for cell (tests/host/test_row_skip_top.cpp), under ASan and UBSan:
seeded windows of 0-600 columns, the two headline pairs in either order of their halves, a 28 | 14 pair (a large length gap
in a three-wave kernel) and an equal-length pair, three scoring schemes, floors of 75 / 85 / 90 % and -- on exact copies,
where every column of W_low is needed and M(r0, j'') is theta exactly -- 100 %, every even row the plan accepts; the
padding rows below the shorter adapter, which nothing may read and the scout may not take; the refusals; the equality
of both layouts' plans for equal lengths; the rule's rows.  No GPU and no HIP involved.

Shown once, each with a temporary edit, to turn the first test red: theta + 1 in row_skip_plan_top (the comparison with row_skip_plan
for equal lengths, the pinned plan of 28 | 22, and the 100 % floors, where the copy reaches theta exactly); W_low four columns short (claim 2, the same copies: the path needs m - r0
columns); the skipping matrix's scout taken through the padding rows (`through` = R: "end cell" / "a pair below F rose",
behind the untracked lead-in)."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_top_aligned_skipping_recurrence_against_the_plain_one():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_row_skip_top")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_row_skip_top.cpp"), "-o", exe])
        out = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        total = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        assert total["bad"] == 0
        # at least every scheme, pair and half at the floors of 90 % (six windows) and 100 % (two): lower floors may leave the
        # row it counts at (the last one above the shorter adapter's end) with theta <= 0 in the longer half
        assert total["pairs"] >= 3 * 6 * (6 + 2) * 2
        # the windows are neither always open nor never
        assert 0 < total["columns_on"] < total["columns"]
        # a scout that took padding rows would have answered otherwise: the exclusion is exercised
        assert total["pad_would_win"] > 0
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("scheme ")]
        assert len(lines) == 3
        for ln in lines:
            count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)}
            assert count["plans"] > 0 and count["at_or_above"] > 0 and count["below"] > 0, ln
        # the rule's rows for the two headline pairs at the default scores: what the shipped kernels are compiled with, and
        # the fastest of the rows measured (profiles/score_top_layout_before_after.txt)
        rule = [ln for ln in out.stdout.splitlines() if ln.startswith("rule ")]
        assert rule == ["rule 28|22=18 33|30=20"], rule


def test_the_rule_is_a_function_of_the_recipe():
    """The seeded simulation answers the same row whichever order the halves come in."""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "r0.cpp")
        exe = os.path.join(tmp, "r0")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "pc_bounds.h"\n'
                    'static void sets(const char *s, unsigned char *o) { for (int i = 0; s[i]; ++i) o[i] = s[i] == \'A\' ? 1 : s[i] == \'C\' ? 2 : s[i] == \'G\' ? 4 : 8; }\n'
                    'int main() { unsigned char a[128], b[128]; sets("AATGTACTTCGTTCAGTTACGTATTGCT", a); sets("GCAATACGTAACTGAACGAAGT", b);\n'
                    'printf("%d %d %d\\n", pcb::row_skip_r0_top(3, -6, -5, -2, 28, 28, 22, a, b), pcb::row_skip_r0_top(3, -6, -5, -2, 28, 22, 28, b, a),\n'
                    'pcb::row_skip_plan_top(3, -6, -5, -2, 28, 18, 28, 22, 58, 46).w_low); return 0; }\n')
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        # 28 | 22 at row 18: ten rows skipped, at the floors of 90 % a window of max(10 + 26 / 2, 4 + 20 / 2) = 23 columns
        assert out.stdout.split() == ["18", "18", "23"]
