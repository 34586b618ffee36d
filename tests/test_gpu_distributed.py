"""The N > 1 path on the one GPU of the test box (functional checks only -- no scaling claim): two ranks over gloo
sharing cuda:0 run the END-TO-END runner with the real HIP library (reads sharded by bases, the presence table
MAX-all-reduced, per-read results gathered in rank order, rank 0 writes): the output files must be the reference CLI's;
and bench.py launched through torch.distributed.run with one rank prints what plain `python bench.py` prints."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["native_default", "native_bins", "ligation_default", "edge_default"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, workdir, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from tests.runner_cases import load_cases, run_case
    cases = load_cases()
    datasets, out = {}, {}
    for name in CASES:
        got = run_case(name, cases[name], os.path.join(workdir, "rank%d" % rank), datasets, device="cuda:0")
        dist.barrier()
        out[name] = got
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_write_the_reference_files(tmp_path):
    from tests.runner_cases import load_cases
    cases = load_cases()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for name in CASES:
        assert got[0][name] == cases[name]["outputs"], (name, got[0][name])
        assert got[1][name] == {}, name          # only rank 0 writes


def _shared_worker(rank, world, port, workdir, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from porechop_amd import runner
    from tests import readgen
    from tests.runner_cases import load_cases, options_from_argv
    cases = load_cases()
    out, shares = {}, {}
    for name in SHARED_CASES:
        case = cases[name]
        box = [readgen.build_dataset(case["dataset"], os.path.join(workdir, "datasets_" + name)) if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        work = os.path.join(workdir, "run_" + name)
        if rank == 0:
            os.makedirs(work)
        dist.barrier()
        target = os.path.join(work, "bins" if case["mode"] == "b" else case["mode"][2:])
        kw = {"options": options_from_argv(case["argv"]), "device": "cuda:0"}
        res = runner.run(box[0], barcode_dir=target, **kw) if case["mode"] == "b" else runner.run(box[0], output=target, **kw)
        dist.barrier()
        out[name] = readgen.output_md5s(target) if rank == 0 else {}
        shares[name] = (len(res.start_trim), res.n_reads)
    q.put((rank, out, shares))
    dist.barrier()
    dist.destroy_process_group()


SHARED_CASES = ["native_default", "native_bins", "native_gz_out", "ligation_default"]


def test_two_ranks_share_one_file_and_each_writes_its_own_span(tmp_path):
    """runner.run_sharded with the real library: both ranks are given the SAME input file and output path (what a multi-GPU
    node does); each parses only the records that start in its half of the bytes and writes its own span of the output.
    The files are the reference CLI's; neither rank held every read."""
    from tests.runner_cases import load_cases
    cases = load_cases()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shared_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        rank, out, shares = q.get(timeout=600)
        got[rank] = (out, shares)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for name in SHARED_CASES:
        assert got[0][0][name] == cases[name]["outputs"], (name, got[0][0][name])
        mine = [got[r][1][name][0] for r in range(2)]
        assert sum(mine) == got[0][1][name][1] and max(mine) < got[0][1][name][1], (name, mine)


def test_one_rank_launcher_equals_plain_bench():
    """`python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` (the driver's launch line) and plain
    `python bench.py`: the same workload, the same results (matching sets, hits, parity), throughput of the same order."""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "200000", "--cpu-seconds", "0", "--no-extra", "--repeats", "1",
            "--full"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    plain = subprocess.run([sys.executable, "bench.py"] + args, cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert plain.returncode == 0, plain.stderr[-2000:]
    launched = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                               "--master-port", str(_free_port()), "bench.py"] + args, cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert launched.returncode == 0, launched.stderr[-2000:]
    a = json.loads(plain.stdout.strip().splitlines()[-1])
    b = json.loads(launched.stdout.strip().splitlines()[-1])
    for k in ("metric", "unit", "n_gpus", "steps", "scaling", "dtype"):
        assert a[k] == b[k], k
    for k in ("workload", "matching_sets", "middle_hits_per_step", "mask_rounds", "world_size"):
        assert a["config"][k] == b["config"][k], k
    assert a["legs"]["exact_prefilter"]["same"] is True and b["legs"]["exact_prefilter"]["same"] is True
    assert a["config"]["pf_same"] is True and b["config"]["pf_same"] is True          # the flat copy the driver's record keeps
    assert len(plain.stdout.strip().splitlines()[-1]) < 8000                          # the whole line fits the driver's 8 KB tail
    # (a sanity band only: these are 3-step runs of a fifth of the benchmark's batch, the first of them on a cold box --
    # observed 0.71 on a fresh box; bench.py's own repeats are the place where throughput is compared)
    assert 1 / 3 < a["value"] / b["value"] < 3, (a["value"], b["value"])


def test_two_ranks_on_one_gpu_emit_the_configs4_leg_for_both_ranks():
    """Multi-GPU readiness (no curve): `bench.py --gpus 2` over gloo, both ranks on the box's one GPU.  The line must carry the
    per-GPU configs[4] shape run by BOTH ranks (n_gpus 2, the exact-prefilter + pruned variant giving the same trims, calls
    and middle hits as the full computation on every rank), both ranks' timed regions, and phase A's check-read shares must
    sum to --check_reads (porechop.py:86)."""
    args = ["--gpus", "2", "--steps", "1", "--warmup", "1", "--reads", "60000", "--reads4", "30000", "--cpu-seconds", "0", "--repeats", "1",
            "--reads4-total", "100000", "--reads-e2e", "40000", "--full"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PC_DIST_BACKEND="gloo")
    # the PLAIN command: bench.py starts its own two ranks (tests/test_bench_launch_cpu.py covers the launch alone)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    run = subprocess.run([sys.executable, "bench.py"] + args, cwd=REPO, env=env, capture_output=True, text=True, timeout=1500)
    assert run.returncode == 0, run.stderr[-3000:]
    line = [l for l in run.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["backend"] == "gloo"
    assert d["config"]["self_launched"] is True and d["config"]["device_by_rank"] == [0, 0] and d["config"]["rccl_world_size_seen"] is None
    assert len(d["config"]["ms_per_step_by_rank"]) == 2
    assert sum(d["config"]["check_reads_by_rank"]) == d["config"]["check_reads"] == 10000
    c4 = d["legs"]["configs4_per_gpu"]
    assert c4["n_gpus"] == 2 and c4["reads_per_gpu"] == 30000
    assert c4["fast_same"] is True and d["config"]["c4_fast_same"] is True
    assert c4["reads_per_s"] > 0 and c4["fast_reads_per_s"] > c4["reads_per_s"]
    # what N GPUs share is in these two (task 5): BASELINE configs[4] as a FIXED total from host memory, and one
    # file in -> one file out over the ranks
    ft = d["legs"]["configs4_fixed_total"]
    assert ft["scaling"] == "strong" and ft["n_gpus"] == 2 and ft["reads_total"] == 100000 and ft["world_size_seen"] == 2
    assert ft["fast_same"] is True and len(ft["ms_by_rank"]) == 2 and sum(ft["check_reads_by_rank"]) == 10000
    assert ft["host_threads_per_rank"] >= 1 and ft["reads_per_s"] > 0
    sf = d["legs"]["sharded_file"]
    assert sf["md5_equal"] is True and sum(sf["reads_by_rank"]) == 40000 and min(sf["reads_by_rank"]) > 0


def test_the_rccl_branch_runs_on_this_box_with_one_rank():
    """backend "nccl" IS RCCL on ROCm.  A single-GPU box cannot hold two RCCL ranks (one device per rank), but a ONE-rank group
    still takes every call of porechop_amd.distributed through the RCCL API: process-group initialisation with a device id (as
    bench.py does), the presence table's float64 MAX all-reduce in place on device tensors (the gloo route copies through the
    host), int64 all_gather / MIN all-reduce of device-staged values, the padded all_gather of gather_in_order, a barrier.
    Until a multi-GPU node runs it this is the only execution the branch gets; two ranks are covered over gloo above."""
    code = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ["PC_DIST_FORCE_COLLECTIVES"] = "1"
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from porechop_amd import distributed as D
assert dist.get_backend() == "nccl" and not D._host_collectives()
dev = torch.device("cuda", 0)
bs = torch.rand(119, dtype=torch.float64, device=dev) * 100
be = torch.rand(119, dtype=torch.float64, device=dev) * 100
rs, re = D.reduce_presence(bs, be)
assert rs.is_cuda and torch.equal(rs, bs) and torch.equal(re, be)
x = torch.arange(12, dtype=torch.int32, device=dev).reshape(6, 2)
assert torch.equal(D.gather_in_order(x), x)
assert D.all_gather_ints([3, 1, 4], dev).tolist() == [[3, 1, 4]]
assert D.all_agree(True, dev) is True and D.all_agree(False, dev) is False
assert D.all_gather_objects({"a": 1}) == [{"a": 1}]
# ... and the sharded route of the runner itself: one file in, one file out, every exchange over RCCL
import hashlib, tempfile
from porechop_amd import runner
from tests import readgen
work = tempfile.mkdtemp(prefix="pc_rccl_")
inp = os.path.join(work, "in.fastq")
open(inp, "w").write(readgen.fastq_text(readgen.native_reads(17, 300, barcodes=(1, 4, 9))))
res = runner.run_sharded(inp, os.path.join(work, "sharded.fastq"), None, runner.Options(), device="cuda:0")
assert res is not None and res.n_reads == 300
dist.barrier()
torch.cuda.synchronize()
dist.destroy_process_group()
one = runner.run(inp, output=os.path.join(work, "single.fastq"), options=runner.Options(), device="cuda:0")
md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
assert md5(os.path.join(work, "sharded.fastq")) == md5(os.path.join(work, "single.fastq")) and one.n_reads == 300
print("rccl one-rank ok", torch.cuda.get_device_name(0))
""" % REPO
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0 and "rccl one-rank ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
