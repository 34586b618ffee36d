"""Compiles porechop_amd/csrc/pc_consensus.h for the HOST and runs tests/host/test_consensus_quality.cpp as a stand-alone program
under ASan and UBSan: pcc's two vote margins (column_margin, slot_margin) and the table index against a naive restatement of
the rule -- every vector of five counters in 0..4 with every template code 0..4 and both tmpl_counts, every four slot counters in
0..3 with voters from their sum to their sum + 4 -- and the hand-stated cases.  No GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_vote_margins_against_the_naive_restatement():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_consensus_quality")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_consensus_quality.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        # 5^5 counter vectors x 5 template codes x 4 bases x 2 tmpl_counts; 4^4 slots x 5 voters x 4 bases
        assert count["cases"] >= 5 ** 5 * 5 * 4 * 2 + 4 ** 4 * 5 * 4
        assert count["slots"] == 4 ** 4 * 5 * 4 and count["columns"] > 0 and count["emitted_slots"] > 0
        assert count["hand"] == 18
