"""Compiles porechop_amd/csrc/pc_paths.h for the HOST, with the device's nibble packing as its memory policy, and replays
every path it returns base by base against the oracle on 30 000 seeded cases of unrestricted schemes
(tests/host/test_paths.cpp), under ASan and UBSan; the same program holds pcs::align_pair (pc_slow.h) and a direct
align_path_window(n, m, 0, n, ...) to align_path on every case.  No GPU involved."""
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_paths_replayed_on_the_host_against_the_oracle():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_paths")
        obj = os.path.join(tmp, "pc_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-std=c11"] + SANITIZE + ["-c", os.path.join(REPO, "oracle", "pc_oracle.c"), "-o", obj])
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + SANITIZE + ["-I", os.path.join(REPO, "porechop_amd", "csrc"),
                               "-I", os.path.join(REPO, "oracle"), os.path.join(REPO, "tests", "host", "test_paths.cpp"),
                               obj, "-o", exe])
        out = subprocess.run([exe, "30000"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "bad=0 " in out.stdout
        keys = ("cases", "linear", "nonnegative_gap", "open_above_extend", "gapped", "empty_path", "rows1", "rows7", "rows8", "rows9", "rows17")
        count = {k: int(out.stdout.split(k + "=")[1].split()[0]) for k in keys}
        assert count["cases"] == 30000
        # every case also went through pcs::align_pair and align_path_window(0, n) and gave the same answer
        assert int(out.stdout.split("one_cell=")[1].split()[0]) == 30000
        # no class went unexercised: the linear dispatch, paths with a gap, empty paths, schemes the packed kernels refuse,
        # and adapters whose last row group of the packed trace holds 1, 7, 8, 1 (of 9) and 1 (of 17) rows
        for k in keys[1:]:
            assert count[k] > 0, (k, out.stdout[-500:])
