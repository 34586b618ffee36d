"""Compiles porechop_amd/csrc/pc_consensus.h for the HOST and runs tests/host/test_consensus.cpp as a stand-alone program under
ASan and UBSan: pcc's banded alignment, traceback and votes against a naive full-matrix implementation -- every pair of strings
over {A, C} of length 0..4 at band 1, 2 and 8, then 5 000 seeded mutated pairs of lengths 1..300 at band 1..64 and 1 000 at band
65..127 --, the banded
distance equal to the plain edit distance whenever band >= max(la, lb) and never below it, and the call rule on hand-stated
counters.  No GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_alignment_traceback_votes_and_call_against_the_full_matrix():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_consensus")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_consensus.cpp"), "-o", exe])
        out = subprocess.run([exe, "5000"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        # 30 templates of length 1..4 x 31 members of length 0..4 x 3 bands
        assert count["exhaustive"] == 30 * 31 * 3 and count["mutated"] == 5000
        assert count["broad"] == 1000 and count["cases"] == count["exhaustive"] + count["mutated"] + count["broad"]
        for key in ("wide", "above", "equal_narrow", "infinite", "with_ins", "with_del", "with_n", "rejected", "accepted"):
            assert count[key] > 0, (key, out.stdout)
        assert count["calls"] == 14


def test_the_rule_header_is_plain_cxx():
    """No device runtime and no other header of the library in the rule: stdint.h is its only include; the traceback order is
    stated in it."""
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_consensus.h")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes == ["stdint.h"], includes
    assert "asm" not in re.sub(r"//.*", "", text)
    assert "TRACEBACK ORDER" in text and "#define PCC_INS_SLOTS 4" in text
