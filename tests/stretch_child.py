"""The scans of tests/test_gpu_stretched_paths.py, one route per child process (TEST INFRASTRUCTURE):
    python -m tests.stretch_child ROUTE DATA [SCHEME_INDEX:JOB,JOB ...]
The library reads its switches (PC_NO_PAIR_TRACE_BOUND, PC_DISABLE_F16, PC_JIT_MIN_CELLS, ...) once per process, so the
parent sets them in the child's environment; DATA is the pickled {scheme: stretchgen.batch(...)} the parent computed once
with the oracle.  ROUTE:
  two_pass   every job of a scheme in ONE PC_MODE_TWO_PASS call (the dual job's tiles of 64 windows and the single jobs'
             tiles of 128 in one launch plan), every record through format_result against the oracle's string;
  trace_at   PC_MODE_SCORE, then PC_MODE_TRACE_AT on its records (window_cap, the ordered buckets); then the same over
             windows that hold nothing but the stretched copy (no longer than the span: window_cap < the bound's window).
A selection "2:0,1" runs jobs 0 and 1 of scheme 2 only (the routes that may compile at run time).  Prints per scheme
pc_trace_ops_x100, at the end pc_jit_stats and STRETCH_OK."""
import ctypes
import os
import pickle
import sys
import time

import numpy as np
import torch

import porechop_amd
from porechop_amd.batch import MODE_SCORE, MODE_TRACE_AT, MODE_TWO_PASS, format_results
from tests import stretchgen as sg


def device_windows(reads):
    arena = torch.from_numpy(np.frombuffer("".join(reads).encode() + b"N" * 64, dtype=np.uint8).copy()).cuda()
    ln = np.array([len(r) for r in reads], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.int64)
    return arena, off, ln


def layout(jobs, names):
    """-> job_adapter, job_adapter_b, job_start, the expected strings in output order (job by job, A's records before B's)"""
    ja, jb, start, want, n = [], [], [0], [], 0
    for j in jobs:
        ja.append(names.index(j["names"][0]))
        jb.append(names.index(j["names"][1]) if j["names"][1] else -1)
        n += len(j["reads"])
        start.append(n)
        for w in j["want"]:
            want += w
    return np.array(ja, dtype=np.int32), np.array(jb, dtype=np.int32), np.array(start, dtype=np.int64), want


def compare(rec, want, what):
    got = format_results(rec)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, (what, len(bad), "records differ; first:", bad[0], got[bad[0]], want[bad[0]])


def main():
    route, data = sys.argv[1], sys.argv[2]
    select = {int(a.split(":")[0]): [int(x) for x in a.split(":")[1].split(",")] for a in sys.argv[3:]}
    with open(data, "rb") as f:
        batches = pickle.load(f)
    forced = int(os.environ.get("PC_FORCE_CHUNKS", "0"))
    lib = porechop_amd.load_library()
    for si, scheme in enumerate(sg.SCHEMES):
        if select and si not in select:
            continue
        t0 = time.time()
        jobs = batches[scheme]
        if select:
            jobs = [jobs[k] for k in select[si]]
        names = sg.adapter_names(scheme)
        ads = [sg.ADAPTERS[n] for n in names]
        if forced:              # pc_api.cpp group_chunks_for must not cap the forced count: the cases sit at ITS boundaries
            assert forced == sg.CHUNKS and sg.N // max(128, max(sg.bounds(scheme, len(a))[2] for a in ads) // 2) >= forced, scheme
        al = porechop_amd.Aligner(ads, scheme)
        reads = [c["read"] for j in jobs for c in j["reads"]]
        arena, off, ln = device_windows(reads)
        assert int(ln.max()) == sg.N
        d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
        ja, jb, start, want = layout(jobs, names)
        out = torch.full((len(want), 8), 77, dtype=torch.int32, device="cuda")
        if route == "two_pass":
            al.scan_device(arena, d_off, d_len, ja, start, sg.N, out, MODE_TWO_PASS, job_adapter_b=jb)
            al.sync()
            compare(out.cpu().numpy(), want, (route, scheme))
        else:
            assert route == "trace_at"
            al.scan_device(arena, d_off, d_len, ja, start, sg.N, out, MODE_SCORE, job_adapter_b=jb)
            al.sync()
            assert bool((out[:, 0] == -2).all())
            al.scan_device(arena, d_off, d_len, ja, start, sg.N, out, MODE_TRACE_AT, job_adapter_b=jb)
            al.sync()
            compare(out.cpu().numpy(), want, (route, scheme))
            # windows no longer than the span, one single-adapter job per adapter
            w_off, w_len, w_want, w_ja, w_start, base = [], [], [], [], [0], 0
            for j in jobs:
                for name, wins, strings in j["tight"]:
                    w_off += [int(off[base + i]) + s for i, s, _ in wins]
                    w_len += [n for _, _, n in wins]
                    w_want += strings
                    w_ja.append(names.index(name))
                    w_start.append(len(w_off))
                base += len(j["reads"])
            t_off = torch.tensor(w_off, dtype=torch.int64, device="cuda")
            t_len = torch.tensor(w_len, dtype=torch.int32, device="cuda")
            cap = max(w_len)
            assert cap < max(sg.bounds(scheme, len(sg.ADAPTERS[j["names"][0]]))[2] for j in jobs)      # window_cap bounds the windows, not ad_window
            rec = torch.full((len(w_off), 8), 77, dtype=torch.int32, device="cuda")
            al.scan_device(arena, t_off, t_len, np.array(w_ja, dtype=np.int32), np.array(w_start, dtype=np.int64), cap, rec, MODE_SCORE)
            al.sync()
            al.scan_device(arena, t_off, t_len, np.array(w_ja, dtype=np.int32), np.array(w_start, dtype=np.int64), cap, rec, MODE_TRACE_AT)
            al.sync()
            compare(rec.cpu().numpy(), w_want, (route, "windows of the span", scheme))
        print("OPS", si, lib.pc_trace_ops_x100(al._ctx), "pairs", len(want), "seconds %.2f" % (time.time() - t0), flush=True)
        c, d = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.pc_jit_stats(ctypes.byref(c), ctypes.byref(d))
        al.close()
    print("JIT", c.value, d.value)
    print("STRETCH_OK", route)


if __name__ == "__main__":
    sys.exit(main())
