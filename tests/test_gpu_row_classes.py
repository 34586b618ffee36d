"""Every row class of the packed DP kernels, launched ALONE at its edges (cases: tests/rowclassgen.py, checked on the CPU by
tests/test_row_class_cases_cpu.py).

The suite's other parity tests send a few hundred windows per adapter length in one call, and pcn::build_table merges such
small groups into the next larger class: four or five of the 39 traced instantiations run.  Here every job is one
pc_scan_device call, so trace16_kernel<R>, scan_kernel<R, PAD, true> and scan_kernel<R, PAD, false> of each class run by
themselves -- which kernel a call launches is what tests/host/plan_probe.cpp says, not what the test believes -- with the lowest
adapter length of the class (most padding rows) and the highest, a full and a 2-pair tile, windows of 1, 2, m - 1, m, m + 1,
149 and 150 columns at every byte alignment, single and dual tiles, packed-fp16 and packed-int16 lanes.  Everything is compared
bit for bit with the oracle: no tolerance anywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import rowclassgen as gen

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = gen.class_labels()


@pytest.fixture(scope="module")
def pa():
    import porechop_amd
    return porechop_amd


@pytest.fixture(scope="module")
def probe():
    return gen.Probe(sanitize=False)          # (the sanitised build is the CPU test's)


@pytest.fixture(scope="module")
def cases(probe):
    return gen.Cases(probe)


@pytest.fixture(scope="module")
def aligner(pa, cases):
    al = pa.Aligner(cases.adapters, cases.scheme)
    yield al
    al.close()


_wanted = {}


def wanted(oracle, job, adapters, scheme):
    """-> (the oracle's strings, its score records (-2, end_j, end_i, 0, score, 0, 0, 0)) of the job's pairs, computed once."""
    key = (job.name, scheme)
    if key not in _wanted:
        strings, rows = [], []
        for w, a in job.pairs():
            strings.append(oracle.adapter_alignment(w, adapters[a], scheme))
            r = oracle.align_raw(w, adapters[a], scheme)
            rows.append([-2, r.end_j, r.end_i, 0, r.score, 0, 0, 0])
        _wanted[key] = (strings, np.array(rows, dtype=np.int32), job.arena)
    assert _wanted[key][2] == job.arena, key                 # (a name stands for one job)
    return _wanted[key][:2]


def scan(al, job, mode):
    dev = torch.device("cuda")
    arena = torch.from_numpy(np.frombuffer(job.arena, dtype=np.uint8).copy()).to(dev)
    off = torch.tensor(job.off, dtype=torch.int64, device=dev)
    ln = torch.tensor(job.wlen, dtype=torch.int32, device=dev)
    n = len(job.windows)
    out = torch.zeros((n * len(job.ad), 8), dtype=torch.int32, device=dev)
    al.scan_device(arena, off, ln, [job.ad[0]], [0, n], job.max_len, out, mode, job_adapter_b=[job.ad[1]] if job.dual else None)
    al.sync()
    return out.cpu().numpy()


def check_traced(pa, rec, job, strings, where):
    pairs = job.pairs()
    assert len(rec) == len(strings) == len(pairs)
    for i, (r, want) in enumerate(zip(rec, strings)):
        got = pa.format_result(r)
        assert got == want, (where, i, len(pairs[i][0]), pairs[i][0], got, want)


def lane_types(rows, probe):
    """(int16_only, ...) to run: classes without a packed-fp16 traced kernel (112, 128) run int16 only."""
    return (False, True) if rows in probe.trace16 else (True,)


def jit_stats(pa):
    compiled, loaded = ctypes.c_int64(0), ctypes.c_int64(0)
    pa.load_library().pc_jit_stats(ctypes.byref(compiled), ctypes.byref(loaded))
    return compiled.value, loaded.value


@pytest.mark.parametrize("label", LABELS)
def test_single_pass_traced(pa, probe, cases, aligner, oracle, label):
    """MODE_TRACE, one call per job: trace16_kernel<R> (as is) and scan_kernel<R, PAD, true> (pc_set_int16_only) of this class
    alone, single and dual tiles; every record is the oracle's, and the two kernels agree byte for byte."""
    cc = cases.by_label[label]
    try:
        for job in cc.end_jobs:
            strings, _ = wanted(oracle, job, cases.adapters, cases.scheme)
            got = {}
            for int16 in lane_types(cc.cls.rows, probe):
                aligner.set_int16_only(int16)
                got[int16] = scan(aligner, job, gen.MODE_TRACE)
                check_traced(pa, got[int16], job, strings, (job.name, "int16" if int16 else "fp16"))
            if len(got) == 2:
                assert got[False].tobytes() == got[True].tobytes(), job.name
    finally:
        aligner.set_int16_only(False)


@pytest.mark.parametrize("label", LABELS)
def test_score_pass(pa, probe, cases, aligner, oracle, label):
    """MODE_SCORE over the same jobs: scan_kernel<R, PAD, false> of this class alone, both lane settings; the records are the
    oracle's end cell and score.  pc_jit_stats does not move: the generic kernel ran, nothing was compiled or loaded."""
    cc = cases.by_label[label]
    before = jit_stats(pa)
    try:
        for job in cc.end_jobs:
            _, rows = wanted(oracle, job, cases.adapters, cases.scheme)
            for int16 in (False, True):
                aligner.set_int16_only(int16)
                rec = scan(aligner, job, gen.MODE_SCORE)
                bad = np.nonzero((rec != rows).any(axis=1))[0]
                assert bad.size == 0, (job.name, int16, int(bad[0]), job.pairs()[int(bad[0])][0], rec[bad[0]].tolist(), rows[bad[0]].tolist())
    finally:
        aligner.set_int16_only(False)
    assert jit_stats(pa) == before


@pytest.mark.parametrize("label", LABELS)
def test_two_pass(pa, probe, cases, aligner, oracle, label):
    """MODE_TWO_PASS over whole reads of window(m) + 40 .. + 200 columns, single and dual, both lane types, against the
    oracle: the score pass (two column chunks where the read is long enough), the planner and the traced pass over the
    bounded window, whose best cells lie before column m, mid-read, one column short of the end and in the last column.
    get_timing()['trace'] counts one timed region per traced launch, which is one per two-pass group: it must be the probe's
    group count for the call, over all the call's pairs."""
    cc = cases.by_label[label]
    aligner.set_timing(True)
    try:
        for job in cc.whole_jobs:
            strings, _ = wanted(oracle, job, cases.adapters, cases.scheme)
            got = {}
            for int16 in lane_types(cc.cls.rows, probe):
                aligner.set_int16_only(int16)
                plan = probe.calls(cases.scheme, [(gen.MODE_TWO_PASS, job.max_len, [job.probe_job()])], int16_only=int16)[0]
                aligner.get_timing()
                got[int16] = scan(aligner, job, gen.MODE_TWO_PASS)
                _, launches, pairs = aligner.get_timing()["trace"]
                assert (launches, pairs) == (len(plan.groups), plan.total), (job.name, int16, launches, pairs, plan)
                check_traced(pa, got[int16], job, strings, (job.name, "int16" if int16 else "fp16"))
            if len(got) == 2:
                assert got[False].tobytes() == got[True].tobytes(), job.name
    finally:
        aligner.set_timing(False)
        aligner.set_int16_only(False)


@pytest.mark.parametrize("scheme,lengths", [(gen.LDS_SCHEMES[0], gen.LDS_LENGTHS), (gen.LDS_SCHEMES[1], gen.LDS_LENGTHS_EPS140),
                                            (gen.LDS_SCHEMES[1], gen.LDS_LENGTHS)])
def test_lds_state_kernel(pa, probe, oracle, scheme, lengths):
    """scan_kernel<0, ...>, the kernel of the schemes that cannot drift: adapters of 1, 2, 127 and 128 bases and the dual
    (1 | 128) under linear gaps, MODE_TRACE over end windows and MODE_TWO_PASS over whole reads, against the oracle.  Under
    (4, -7, -10, -140) the packed kernels take a panel of up to 57 bases only (pcb::scores_supported), so the LDS-state kernel
    gets 1, 2, 56, 57 and (1 | 57) there; the lengths 1, 2, 127, 128 run all the same and take the plain-int32 kernel
    (tests/test_row_class_cases_cpu.py holds both facts from the probe)."""
    cs = gen.LdsCases(probe, scheme, lengths)
    al = pa.Aligner(cs.adapters, scheme)
    try:
        for jobs, mode in ((cs.end_jobs, gen.MODE_TRACE), (cs.whole_jobs, gen.MODE_TWO_PASS)):
            for job in jobs:
                strings, _ = wanted(oracle, job, cs.adapters, scheme)
                check_traced(pa, scan(al, job, mode), job, strings, (job.name, mode))
    finally:
        al.close()


def test_fp16_gate_at_its_column_limit(probe):
    """tests/row_class_gate_child.py, the one child process: PC_CHECK_RANGE=1 is read once per process (the range-checking
    build of trace16_kernel records the extremes of every value it forms; it never traps).  Windows of exactly max_cols
    columns run the packed-fp16 kernel with every value within +-2040, windows one column longer the packed-int16 kernel,
    and both give the oracle's records."""
    env = dict(os.environ, PC_CHECK_RANGE="1")
    for k in ("PC_DISABLE_F16", "PC_DEBUG_TRACE", "PC_NO_MERGE_SMALL", "PC_NO_SPLIT_DUAL"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "tests.row_class_gate_child", probe.exe], capture_output=True, text=True, env=env,
                         timeout=600, cwd=REPO)
    assert res.returncode == 0 and "GATE_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-4000:]
    # every admitted class of both schemes, at and above its limit
    admitted = sum(1 for scheme in gen.GATE_SCHEMES for r in probe.trace16 if probe.f16(scheme, r, 1)[1] > 0)
    assert res.stdout.count("AT_LIMIT") == res.stdout.count("ABOVE_LIMIT") == admitted == 14 + 8, res.stdout[-3000:]
