"""Compiles porechop_amd/csrc/pc_prefilter_plan.h for the HOST and interprets the plans it builds -- the exhaustive stage and
the seed stage, in plain C++ -- against the oracle's edit distance on 600 seeded cases, for the three routes and the four
option settings (tests/host/test_prefilter_plan.cpp), under ASan and UBSan.  No GPU involved."""
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_plans_interpreted_on_the_host_against_the_oracle():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_prefilter_plan")
        obj = os.path.join(tmp, "pc_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-std=c11"] + SANITIZE + ["-c", os.path.join(REPO, "oracle", "pc_oracle.c"), "-o", obj])
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               "-I", os.path.join(REPO, "oracle"), os.path.join(REPO, "tests", "host", "test_prefilter_plan.cpp"),
                               obj, "-o", exe])
        out = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(out.stdout.split(k + "=")[1].split()[0]) for k in ("cases", "seeded", "rest", "long")}
        assert count["cases"] == 600
        # no class went unexercised: pieces the seed stage took, pieces left to the exhaustive kernel, and pairs of adapters
        # above 32 bases that lie within their bound
        assert count["seeded"] > 0 and count["rest"] > 0 and count["long"] > 0
