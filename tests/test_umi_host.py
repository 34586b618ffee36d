"""Compiles porechop_amd/csrc/pc_umi.h for the HOST and runs tests/host/test_umi.cpp as a stand-alone program under ASan and
UBSan: pcu::span, pcu::extract and pcu::qualifies over about 20 000 seeded (window, adapter) pairs whose paths come from
pcpath::align_path_sets, the routine the device runs per lane.  No GPU and no HIP involved."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_extract_and_qualifies_against_a_naive_replay():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_umi")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_umi.cpp"), "-o", exe])
        out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        count = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.splitlines()[-1])}
        assert count["cases"] >= 20000
        for key in ("status0", "status1", "status2", "status3", "len0", "len_above", "len_below", "qualifies", "not", "gapped_in_span",
                    "row0", "lastrow", "single", "whole", "blocks", "plant_whole", "clip_left", "clip_right", "sub", "ins", "del",
                    "absent", "several"):
            assert count[key] > 0, (key, out.stdout)


def test_the_umi_header_is_plain_cxx():
    """No device runtime and no other header of the library in the rule: stdint.h is its only include."""
    text = open(os.path.join(REPO, "porechop_amd", "csrc", "pc_umi.h")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes == ["stdint.h"], includes
    assert "asm" not in re.sub(r"//.*", "", text)
