"""Compiles porechop_amd/csrc/pc_middle_paths.h for the HOST, with the device's nibble packing as its memory policy, and
compares the path it finds inside a hit's bounded window with pcpath::align_path over the whole, explicitly masked read
(tests/host/test_middle_paths.cpp), under ASan and UBSan.  No GPU involved.

Beside the program's own seeded reads it gets the gap-stretched copies of tests/stretchgen.py -- tight-pair, widest,
truncated, start and start-cut, for every scheme and adapter of the generator -- so that paths as wide as W and windows
with a full warm-up occur; the random cases alone stay tens of columns away from the bounds."""
import os
import random
import subprocess
import tempfile

from tests import stretchgen as sg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
RANDOM_CASES = 3000


def stretched_lines(oracle):
    lines = []
    for k, scheme in enumerate(sg.SCHEMES):
        for name in sg.adapter_names(scheme):
            rng = random.Random(7000 + 10 * k + len(name))
            for c in sg.stretched_cases(oracle, rng, scheme, name):
                lines.append("%s %s %d %d %d %d" % ((c["read"], sg.ADAPTERS[name]) + tuple(scheme)))
    return lines


def test_windowed_paths_equal_whole_read_paths_on_the_host(oracle):
    lines = stretched_lines(oracle)
    assert len(lines) > 500
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_middle_paths")
        cases = os.path.join(tmp, "cases.txt")
        with open(cases, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               os.path.join(REPO, "tests", "host", "test_middle_paths.cpp"), "-o", exe])
        out = subprocess.run([exe, str(RANDOM_CASES), "12345", cases], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "bad=0 " in out.stdout
    print(out.stdout)
    # c0 > 0 with c1 < n; c0 == 0; c1 == n with I < m; a mask inside the window, astride c0, astride c1; a hit next to a
    # mask; a path within 2 columns of W; the linear dispatch; a refused scheme (window = whole read); every adapter length
    keys = ("interior", "c0_zero", "cut_by_end", "mask_inside", "mask_astride_c0", "mask_astride_c1", "mask_adjacent", "near_W",
            "linear", "open_above_extend", "refused") + tuple("rows%d" % m for m in (1, 7, 8, 9, 17, 28, 33, 68, 111))
    count = {k: int(out.stdout.split(" " + k + "=")[1].split()[0]) for k in keys + ("from_file", "skipped")}
    assert count["from_file"] == len(lines)
    assert int(out.stdout.split("cases=")[1].split()[0]) + count["skipped"] == RANDOM_CASES + 2 * len(lines)
    for k in keys:
        assert count[k] > 0, (k, out.stdout[-800:])
