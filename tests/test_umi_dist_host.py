"""Compiles porechop_amd/csrc/pc_umi_dist.h for the HOST and runs tests/host/test_umi_dist.cpp as a stand-alone program under
ASan and UBSan: pcud::distance at both word widths against the plain DP -- every pair of strings of length 0..5, then 20 000
seeded random and mutated pairs at the lengths where a width or a mask ends, garbage above every key's length -- and
pcud::lower_bound <= distance on all of them, each of its three terms binding somewhere.  No GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_distance_and_lower_bound_against_the_plain_dp():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_umi_dist")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_umi_dist.cpp"), "-o", exe])
        out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        assert count["exhaustive"] == 1365 * 1365 and count["mutated"] + count["random"] >= 20000
        assert count["cases"] == count["bound_ok"] == count["wide"]
        for key in ("narrow", "bind_len", "bind_plus", "bind_minus", "tight", "slack", "empty", "full64", "mutated", "random"):
            assert count[key] > 0, (key, out.stdout)


def test_the_distance_header_is_plain_cxx():
    """No device runtime and no other header of the library in the rule: stdint.h is its only include."""
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_umi_dist.h")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes == ["stdint.h"], includes
    assert "asm" not in re.sub(r"//.*", "", text)
