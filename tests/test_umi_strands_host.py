"""Compiles the both-strands rule for the HOST and runs tests/host/test_umi_strands.cpp as a stand-alone program under ASan and
UBSan: pcud::mirror against a per-base loop at every length 0..64 and mirror(mirror(k)) == k, the mirrored-composition bound
never above the true d(a, mirror(b)) on 20 000 seeded pairs, pcc::comp_code on all 256 bytes, and pcc::fill / walk / votes of a
member handed over reversed and complemented against those of the materialised reverse complement.  No GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_mirror_bound_and_reverse_complemented_members():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_umi_strands")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_umi_strands.cpp"), "-o", exe])
        out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        assert count["mirrors"] == 65 * 40 + 1 and count["pairs"] == 20000 == count["bound_ok"] and count["codes"] == 256
        assert count["pileups"] == 402
        for key in ("bound_tight", "bound_binds", "planted", "accepted", "with_n"):
            assert count[key] > 0, (key, out.stdout)
