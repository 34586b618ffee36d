"""Compiles porechop_amd/csrc/pc_end_rule.h for the HOST and checks the rule phase B hands to the end-window scan against the
oracle (tests/host/test_end_rule.cpp), under ASan and UBSan: every pair the rule rejects from its score record has trim 0
by the reference's condition, the rule's bound holds for the pairs it keeps, and in each of the three scoring schemes it
rejects some pairs and keeps some.  The same function the device runs between the two passes; no GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_rejected_pairs_do_not_trim_under_the_oracle():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_end_rule")
        obj = os.path.join(tmp, "pc_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-std=c11"] + SANITIZE + ["-c", os.path.join(REPO, "oracle", "pc_oracle.c"), "-o", obj])
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               "-I", os.path.join(REPO, "oracle"), os.path.join(REPO, "tests", "host", "test_end_rule.cpp"), obj, "-o", exe])
        out = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        assert int(out.stdout.split("pairs=")[1].split()[0]) >= 3 * 2 * 5 * 2 * 7 * 40
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("scheme ")]
        assert len(lines) == 3
        for ln in lines:
            count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)}
            assert count["rejected"] > 0 and count["accepted"] > 0 and count["trimming"] > 0, ln


def test_plan_decisions_of_a_scan_with_an_end_rule():
    """pc_scan_plan.h on the host (tests/host/test_end_rule_plan.cpp): short windows go through two passes under PC_MODE_AUTO
    with a rule and only then; the two-pass groups carry each segment's first window and adapter; which groups take the route."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_end_rule_plan")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_end_rule_plan.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "bad=0 " in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_the_rule_header_is_plain_cxx():
    """No device runtime in the rule: it is what the host test above, the planner's kernels and any caller can hold."""
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_end_rule.h")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes == ["stdint.h"], includes
