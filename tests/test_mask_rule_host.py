"""Compiles porechop_amd/csrc/pc_mask_rule.h for the HOST and checks the rule the mask rounds of the middle scan rest on
against the oracle (tests/host/test_mask_rule.cpp), under ASan and UBSan: after a mask no score rises, every record the rule
keeps is the oracle's record of the masked read, a pair below its floor stays below, the rule keeps at least a quarter and
realigns at least a tenth of the pairs in each of the three scoring schemes, and the gate refuses what the claim does not
cover.  The same functions the selection kernel runs; no GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_kept_records_are_the_oracles_after_the_mask():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_mask_rule")
        obj = os.path.join(tmp, "pc_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-std=c11"] + SANITIZE + ["-c", os.path.join(REPO, "oracle", "pc_oracle.c"), "-o", obj])
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               "-I", os.path.join(REPO, "oracle"), os.path.join(REPO, "tests", "host", "test_mask_rule.cpp"), obj, "-o", exe])
        out = subprocess.run([exe, "150"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        assert "the N adapter: 47 -> 81" in out.stdout
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("scheme ")]
        assert len(lines) == 3
        for ln in lines:
            count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)}
            judged = count["kept"] + count["realigned"]
            assert count["cases"] >= 6 * 6 * 150 and count["bad"] == 0, ln
            assert 4 * count["kept"] >= judged and 10 * count["realigned"] >= judged and (count["below_floor"] > 0 or count["floors"] == 0), ln
        assert sum("floors=0 " not in ln for ln in lines) >= 2            # (4, -7, -10, -140 gives no floor: a gap costs more than 140 bases earn)


def test_the_rule_header_is_plain_cxx():
    """No device runtime in the rule: it is what the host test above, the selection kernel and any caller can hold."""
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_mask_rule.h")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes == ["stdint.h"], includes
