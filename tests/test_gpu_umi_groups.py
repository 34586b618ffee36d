"""UMI neighbours on the MI355X (pc_umi_neighbours / Aligner.umi_neighbours, csrc/pc_umi_groups.hip) against the numpy model
umi_groups.neighbours_host -- itself checked against the plain DP in tests/test_umi_groups_cpu.py -- and the runner's grouping
on the library.  The model runs ONCE per key set, at max_dist 64 over all 600 keys: every smaller n and max_dist is a filter of
those rows."""
import ctypes
import random

import numpy as np
import pytest

from porechop_amd import umi_groups as ug

pytestmark = pytest.mark.gpu

BAD_ARG = -3
N_ALL = 600
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 600]      # the wave's and the tile's edges; 600: three tiles, the last one ragged
DISTS = [0, 1, 2, 5, 64]


def _mutate(rng, key, edits, fixed=None):
    k = list(key)
    for _ in range(edits):
        kind, at = rng.randrange(3), rng.randrange(len(k) + 1)
        if kind == 0 and k:
            k[min(at, len(k) - 1)] = rng.choice("ACGT")
        elif kind == 1 and len(k) < 64:
            k.insert(at, rng.choice("ACGT"))
        elif k:
            del k[min(at, len(k) - 1)]
    if fixed is not None:
        k = (k + [rng.choice("ACGT") for _ in range(fixed)])[:fixed]
    return "".join(k)


def _keys(name):
    """600 keys: seeded originals, each followed by copies mutated by a known number of edits (1 .. 6)."""
    rng = random.Random({"short": 32, "mixed": 64, "long": 6464, "dups": 2}[name])
    lengths = {"short": [22] * 6 + [0, 1, 31, 32], "mixed": list(range(65)), "long": [64], "dups": [22, 22, 22, 0, 40]}[name]
    keys = []
    while len(keys) < N_ALL:
        original = "".join(rng.choice("ACGT") for _ in range(rng.choice(lengths)))
        keys.append(original)
        for edits in rng.sample(range(1, 7), 3):
            copy = _mutate(rng, original, edits, 64 if name == "long" else None)
            keys.append(copy if name != "short" or len(copy) <= 32 else copy[:32])
        if name == "dups":
            keys += [original] * rng.randrange(1, 4) + [keys[-1]]
    keys = keys[:N_ALL]
    rng.shuffle(keys)
    return keys


class KeySet:
    def __init__(self, name):
        self.keys = _keys(name)
        self.planes, self.lens = ug.pack(self.keys)
        self.all = ug.neighbours_host(self.planes, self.lens, 64)          # every pair with its distance: the model, once
        assert self.all.shape[0] == N_ALL * (N_ALL - 1) // 2

    def want(self, n, max_dist):
        a = self.all
        return a[(a[:, 1] < n) & (a[:, 2] <= max_dist)]

    def device(self, n=N_ALL, planes=None):
        import torch
        p = self.planes if planes is None else planes
        return (torch.from_numpy(np.ascontiguousarray(p[:n]).view(np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(self.lens[:n])).cuda())


@pytest.fixture(scope="module")
def sets():
    made = {}

    def get(name):
        if name not in made:
            made[name] = KeySet(name)
        return made[name]
    return get


@pytest.fixture(scope="module")
def al():
    import porechop_amd
    from tests.umigen import SCHEMES
    a = porechop_amd.Aligner(["ACGTACGTACGT"], SCHEMES["default"])
    yield a
    a.close()


def test_the_key_sets_are_what_they_claim(sets):
    assert sets("short").lens.max() == 32 and sets("long").lens.min() == 64 and sets("long").lens.max() == 64
    mixed = sets("mixed").lens
    assert mixed.min() == 0 and mixed.max() == 64 and (mixed > 32).sum() > 100 and (mixed <= 32).sum() > 100
    dups = sets("dups")
    assert (dups.all[:, 2] == 0).sum() > 200


@pytest.mark.parametrize("max_dist", DISTS)
@pytest.mark.parametrize("name", ["short", "mixed", "long", "dups"])
def test_neighbours_equal_the_model(sets, al, name, max_dist):
    ks = sets(name)
    if max_dist in (1, 2, 5):          # asserted on the model before the GPU is asked: the case cannot go vacuous
        d = ks.all[:, 2]
        assert (d == max_dist).sum() >= 20 and (d == max_dist + 1).sum() >= 20, ((d == max_dist).sum(), (d == max_dist + 1).sum())
    for n in SIZES:
        planes, lens = ks.device(n)
        got = al.umi_neighbours(planes, lens, max_dist)
        want = ks.want(n, max_dist)
        assert got.is_cuda and str(got.dtype) == "torch.int32" and tuple(got.shape) == want.shape, (name, n, max_dist, tuple(got.shape), want.shape)
        assert np.array_equal(got.cpu().numpy(), want), (name, n, max_dist)


@pytest.mark.parametrize("name", ["short", "mixed", "long", "dups"])
def test_without_the_prunes_the_same_pairs(sets, al, name, monkeypatch):
    ks = sets(name)
    planes, lens = ks.device()
    monkeypatch.setenv("PC_UMI_NO_PRUNE", "1")
    for max_dist in (0, 2):
        assert np.array_equal(al.umi_neighbours(planes, lens, max_dist).cpu().numpy(), ks.want(N_ALL, max_dist))
    monkeypatch.delenv("PC_UMI_NO_PRUNE")
    assert np.array_equal(al.umi_neighbours(planes, lens, 2).cpu().numpy(), ks.want(N_ALL, 2))


@pytest.mark.parametrize("name", ["short", "mixed"])
def test_garbage_above_the_length_changes_nothing(sets, al, name):
    ks = sets(name)
    rng = np.random.default_rng(5)
    above = ~ug._len_mask(ks.lens)[:, None]
    dirty = ks.planes | (rng.integers(0, 2**64 - 1, size=ks.planes.shape, dtype=np.uint64, endpoint=True) & above)
    if name == "short":
        dirty[:, :] |= np.where(ks.lens[:, None] < 32, np.uint64(1) << np.uint64(63), np.uint64(0))     # bits above the 32-bit word too
    assert (dirty != ks.planes).any()
    planes, lens = ks.device(planes=dirty)
    for max_dist in (0, 2, 5):
        assert np.array_equal(al.umi_neighbours(planes, lens, max_dist).cpu().numpy(), ks.want(N_ALL, max_dist))


def _raw(al, planes, lens, n, max_len, max_dist, pairs, cap, found):
    import torch
    return al.lib.pc_umi_neighbours(al._ctx, planes.data_ptr(), lens.data_ptr(), n, max_len, max_dist, pairs.data_ptr(), cap,
                                    found.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_a_cap_below_found(sets, al):
    import torch
    ks = sets("dups")
    planes, lens = ks.device()
    want = ks.want(N_ALL, 2)
    cap = want.shape[0] // 3
    assert cap > 100
    pairs = torch.full((cap + 8, 3), -7, dtype=torch.int32, device="cuda")
    found = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    assert _raw(al, planes, lens, N_ALL, 64, 2, pairs, cap, found) == 0
    al.sync()
    assert int(found.item()) == want.shape[0]                               # exact, whatever fitted
    rows = pairs.cpu().numpy()
    assert (rows[cap:] == -7).all()                                         # nothing behind the cap
    written = {tuple(r) for r in rows[:cap].tolist()}
    assert len(written) == cap and written <= {tuple(r) for r in want.tolist()}
    # the wrapper never hands an incomplete list on
    assert np.array_equal(al.umi_neighbours(planes, lens, 2, cap=cap).cpu().numpy(), want)
    assert np.array_equal(al.umi_neighbours(planes, lens, 2, cap=0).cpu().numpy(), want)
    # cap == 0 with no room at all: only the count
    assert _raw(al, planes, lens, N_ALL, 64, 2, pairs, 0, found) == 0
    al.sync()
    assert int(found.item()) == want.shape[0] and (pairs.cpu().numpy()[cap:] == -7).all()


def test_refusals_write_nothing(sets, al):
    import torch
    ks = sets("short")
    planes, lens = ks.device()
    pairs = torch.full((1024, 3), -7, dtype=torch.int32, device="cuda")
    found = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    for kw in (dict(n=-1), dict(n=1 << 31), dict(max_len=-1), dict(max_len=65), dict(max_dist=-1), dict(max_dist=65), dict(cap=-1)):
        args = dict(n=N_ALL, max_len=32, max_dist=2, cap=1024)
        args.update(kw)
        assert _raw(al, planes, lens, args["n"], args["max_len"], args["max_dist"], pairs, args["cap"], found) == BAD_ARG, kw
        al.sync()
        assert int(found.item()) == 77 and int((pairs != -7).sum()) == 0, kw
    # n < 2: the counter is zeroed and nothing else happens
    for n in (0, 1):
        found.fill_(77)
        assert _raw(al, planes, lens, n, 32, 2, pairs, 1024, found) == 0
        al.sync()
        assert int(found.item()) == 0 and int((pairs != -7).sum()) == 0
    # and the context goes on working
    assert np.array_equal(al.umi_neighbours(planes, lens, 1).cpu().numpy(), ks.want(N_ALL, 1))


def test_a_length_above_max_len_is_reported_and_has_no_pairs(sets, al):
    """As test_gpu_umi.py does for a window above max_len: the kernel counts the key, gives it no pairs and reads nothing of it
    beyond its two planes; the error surfaces at sync()."""
    import torch
    ks = sets("short")
    planes, lens = ks.device()
    long_ones = np.nonzero(ks.lens > 22)[0]
    assert 0 < long_ones.size < N_ALL - 100
    pairs = torch.full((8192, 3), -7, dtype=torch.int32, device="cuda")
    found = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert _raw(al, planes, lens, N_ALL, 22, 2, pairs, 8192, found) == 0
    with pytest.raises(RuntimeError):
        al.sync()
    want = ks.want(N_ALL, 2)
    want = want[~np.isin(want[:, 0], long_ones) & ~np.isin(want[:, 1], long_ones)]
    m = int(found.item())
    assert m == want.shape[0] and m <= 8192
    got = pairs[:m].cpu().numpy()
    assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want)
    # a length no kernel takes: the wrapper passes max_len 64, and the key is reported the same way
    bad = ks.lens.copy()
    bad[7] = 70
    with pytest.raises(RuntimeError):
        al.umi_neighbours(planes, torch.from_numpy(bad).cuda(), 2)
    assert np.array_equal(al.umi_neighbours(planes, lens, 2).cpu().numpy(), ks.want(N_ALL, 2))      # after the report


def test_the_route_of_the_rule_orders_by_length_and_maps_back(sets, al):
    ks = sets("mixed")
    for max_dist in (0, 2, 5):
        assert np.array_equal(ug.neighbours(ks.planes, ks.lens, max_dist, al), ks.want(N_ALL, max_dist))


# ---- the runner on the library: the TSV the host route writes -----------------------------------------------------------------
def test_runner_writes_the_groups_the_host_route_writes(tmp_path):
    from porechop_amd import runner
    from tests import umi_groups_aligner as gcase
    from tests import umi_runner_case
    inp = tmp_path / "reads.fastq"
    inp.write_text(umi_runner_case.fastq_text(gcase.build()))
    opts = runner.Options()
    opts.check_reads = 3
    for tag, streamed in (("whole", None), ("streamed", 4000)):
        out, tsv, plain = tmp_path / ("out_%s.fastq" % tag), tmp_path / ("groups_%s.tsv" % tag), tmp_path / ("plain_%s.fastq" % tag)
        kw = dict(adapter_panel=umi_runner_case.adapter_sets(), wildcards=True, umi=True)
        if streamed:
            res = runner.run_streamed(str(inp), str(out), None, opts, block_bytes=streamed, umi_groups=str(tsv), **kw)
            assert res is not None, "not streamed"
            runner.run_streamed(str(inp), str(plain), None, opts, block_bytes=streamed, **kw)
        else:
            res = runner.run(str(inp), output=str(out), options=opts, umi_groups=str(tsv), **kw)
            runner.run(str(inp), output=str(plain), options=opts, **kw)
        assert tsv.read_text() == gcase.groups_text(gcase.ROWS_BOTH), tag
        assert res.umi_groups == gcase.GROUPS_BOTH
        assert out.read_bytes() == plain.read_bytes()
    # the host route on the same UMIs
    per_read, rows = ug.assign(res.umis, ["read_%d" % (k + 1) for k in range(10)], "both")
    assert per_read == gcase.GROUPS_BOTH and ug.groups_header() + rows == gcase.groups_text(gcase.ROWS_BOTH)
