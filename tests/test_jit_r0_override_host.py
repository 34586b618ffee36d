"""PC_JIT_R0, the measurement switch that replaces the rule's row of the row-skipping score kernel: its text is read by
pcb::row_skip_r0_override (csrc/pc_bounds.h), compiled here for the HOST under ASan and UBSan.  One row for every pair, or a
row per pair named by both of its lengths; a pair that is not listed keeps the rule's row; malformed text is reported and
ignored as a whole."""
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# (text, m_a, m_b) -> (row, malformed) with the rule's row 20
CASES = [
    ("22", 28, 22, 22, 0), ("0", 28, 22, 0, 0), ("18", 33, 30, 18, 0),
    ("28|22:22,33|30:18", 28, 22, 22, 0), ("28|22:22,33|30:18", 33, 30, 18, 0), ("28|22:22,33|30:18", 30, 33, 18, 0),
    ("28|22:22,33|30:18", 24, 24, 20, 0),                       # not listed: the rule's row
    ("28|22:22,28|24:16", 28, 24, 16, 0), ("28|22:22,28|24:16", 28, 22, 22, 0),      # two pairs with the same longer adapter
    ("", 28, 22, 20, 1), ("abc", 28, 22, 20, 1), ("28:22", 28, 22, 20, 1), ("28|22:", 28, 22, 20, 1), ("28|22:22,", 28, 22, 20, 1),
    ("28|22:22;33|30:18", 28, 22, 20, 1), ("28|22:22,33|30", 28, 22, 20, 1), ("22 ", 28, 22, 20, 1), ("28|22:-4", 28, 22, 20, 1),
]


def test_rows_per_pair_and_malformed_text():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "r0.cpp"), os.path.join(tmp, "r0")
        lines = ['{ bool bad = false; const int v = pcb::row_skip_r0_override("%s", %d, %d, 20, &bad); printf("%%d %%d\\n", v, (int)bad); }'
                 % (t, a, b) for t, a, b, _, _ in CASES]
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "pc_bounds.h"\nint main() {\n' + "\n".join(lines) + "\nreturn 0; }\n")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        got = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
        assert got == [(row, bad) for _, _, _, row, bad in CASES], list(zip(CASES, got))
