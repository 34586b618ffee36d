"""Compiles porechop_amd/csrc/pc_scan_plan.h for the HOST and checks the plans it makes -- tables, chunks and grids, scratch
layout, score launches -- on 400 job lists over every mode, four scoring schemes and both table options
(tests/host/test_scan_plan.cpp), under ASan and UBSan.  The runs are expanded with the function the device's expansion
kernel calls.  No GPU and no HIP involved."""
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CLASSES = ("merge", "split", "slow", "generic", "tail", "ragged")


def test_scan_plans_checked_on_the_host():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_scan_plan")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_scan_plan.cpp"), "-o", exe])
        out = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(out.stdout.split(k + "=")[1].split()[0]) for k in ("lists",) + CLASSES}
        assert count["lists"] >= 400
        # no class went unexercised: a merge of small groups, a split two-adapter job, a plain-int32 job, a generic group, a
        # chunked tail and a chunking by the ragged rule
        assert all(count[k] > 0 for k in CLASSES), count


def test_the_plan_header_is_host_only():
    """No device runtime and no environment in the plan: it is what the host test above can hold."""
    import re
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_scan_plan.h")).read()
    assert not re.search(r"\b(hip\w*|getenv|pc_ctx)\b", text)
