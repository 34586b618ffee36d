"""The gap-stretched cases of tests/stretchgen.py, checked on the host with the oracle alone: every case respects the bounds
of csrc/pc_bounds.h (restated in stretchgen.bounds / pair_bound), some cases MEET them -- otherwise the GPU tests
(tests/test_gpu_stretched_paths.py) would again stay tens of columns away from where the kernels stop recording trace --
and the placements and tiles are what those tests assume.

The per-pair bound (without plan_kernel's + 2) minus the path's span is (|open| - g) // g on every tight-pair case: 0 for
(3,-6,-2,-5), (5,-4,-10,-40), (4,-7,-10,-140) and the linear schemes, 1 for (3,-6,-5,-2) and (20,-30,-25,-12), 9 for
(5,-4,-10,-1).  Smallest W - span reached per scheme, as measured on the oracle (asserted for the first two only; the others are
what the search finds, written down):
    (3,-6,-5,-5)      0   (every adapter)          asserted: == 0
    (3,-6,-2,-5)      1   (22-mer, 33-mer)         asserted: <= 1
    (4,-7,-10,-140)   0   (every adapter)
    (5,-4,-10,-40)    0   (33-mer)
    (1,-1,-1,-1)      1
    (20,-30,-25,-12)  2
    (3,-6,-5,-2)      3   (33-mer; the larger piece alone, the other rows deleted, beats a wider path)
    (5,-4,-10,-1)    30   (22-mer; likewise: W = 6 m assumes a path of score 0)"""
import pytest

from tests import stretchgen as sg


@pytest.fixture(scope="module")
def batches(oracle):
    return {sc: sg.batch(oracle, sc) for sc in sg.SCHEMES}


def stretched_cases(jobs):
    seen = set()
    for job in jobs:
        for c in job["reads"]:
            if c["kind"] == "stretched" and id(c) not in seen:
                seen.add(id(c))
                yield c


def test_schemes_adapters_and_chunks_are_the_ones_asked_for():
    assert set(sg.SCHEMES) == {(3, -6, -5, -2), (3, -6, -2, -5), (5, -4, -10, -1), (20, -30, -25, -12), (5, -4, -10, -40), (4, -7, -10, -140),
                               (3, -6, -5, -5), (1, -1, -1, -1)}
    assert [len(sg.ADAPTERS[n]) for n in sg.adapter_names(sg.DEFAULT)] == [28, 22, 33, 68, 111]
    for sc in sg.SCHEMES:
        names = sg.adapter_names(sc)
        assert names[:3] == ["Y_Top", "Y_Bottom", "A33"] and ("A111" in names) == (sc == sg.DEFAULT)
        assert ("A68" in names) == (sc != sg.NO_DRIFT)                      # (outside the packed kernels' range there)
        # PC_FORCE_CHUNKS=4 is not capped by group_chunks_for: max_len / max(128, window / 2) >= 4 for the widest window
        assert sg.N // max(128, max(sg.bounds(sc, len(sg.ADAPTERS[n]))[2] for n in names) // 2) >= sg.CHUNKS, sc
    for n in ("A33", "A68", "A111"):
        s = sg.ADAPTERS[n]
        assert all(a != b for a, b in zip(s, s[1:]))
    assert sg.CHUNK_LEN * sg.CHUNKS == sg.N and sg.BOUNDARIES == (480, 960, 1440)
    # a filler differs from both of its neighbours
    ad = sg.ADAPTERS["A33"]
    s = sg.stretched(ad, [11, 22], 7)
    assert len(s) == 33 + 14 and s[:11] == ad[:11] and s[18:29] == ad[11:22] and s[36:] == ad[22:]
    for k in list(range(11, 18)) + list(range(29, 36)):
        assert s[k] != s[k - 1] and s[k] != s[k + 1]


@pytest.mark.parametrize("scheme", sg.SCHEMES)
def test_every_case_respects_the_bounds_and_some_meet_them(batches, scheme):
    g = min(-scheme[2], -scheme[3])
    tight_slack, w_slack = {}, {}
    for c in stretched_cases(batches[scheme]):
        f, m = c["facts"], len(sg.ADAPTERS[c["adapter"]])
        W = sg.bounds(scheme, m)[0]
        assert not f.failed and f.ae == f.I - 1 and f.score > 0
        if c["family"] == "start-cut":                      # the path runs down column 0 first: it touches J columns
            assert f.rs == 0 and f.a_s == c["cut"] and m < f.J < c["full_span"]
        else:
            assert sg.covers(f, m)
        assert (f.I < m) == (c["family"] == "truncated")
        if c["family"] == "start":
            assert f.rs == 0 and f.J == f.span
        assert f.span <= f.I + max(0, scheme[0] * f.I - f.score) // g == sg.pair_bound(scheme, f.I, f.score), c
        assert f.span <= W, c
        if c["family"] == "tight-pair":
            tight_slack[c["adapter"]] = min(tight_slack.get(c["adapter"], 1 << 30), sg.pair_bound(scheme, f.I, f.score) - f.span)
        w_slack[c["adapter"]] = min(w_slack.get(c["adapter"], 1 << 30), W - f.span)
    names = sg.adapter_names(scheme)
    assert sorted(tight_slack) == sorted(names)
    for n in names:
        assert tight_slack[n] <= (-scheme[2] - g) // g, (n, tight_slack)
    print("W - span", scheme, w_slack)
    if scheme == (3, -6, -5, -5):
        assert min(w_slack.values()) == 0, w_slack
    if scheme == (3, -6, -2, -5):
        assert min(w_slack.values()) <= 1, w_slack


@pytest.mark.parametrize("scheme", sg.SCHEMES)
def test_placements_and_tiles(batches, scheme):
    jobs = batches[scheme]
    assert [j["names"] for j in jobs] == sg.jobs_for(scheme) + sg.pure_jobs_for(scheme)
    assert [j["pure"] for j in jobs] == [False] * len(sg.jobs_for(scheme)) + [True] * len(sg.pure_jobs_for(scheme))
    for job in jobs:
        if job["pure"]:         # one tile (two halves of 64) of full-length pass-2 windows, stretched pairs alone, the widest among them
            m = len(job["ads"][0])
            W, _, window, g = sg.bounds(scheme, m)
            cases = job["reads"]
            assert 40 <= len(cases) <= 2 * sg.TILE and all(c["kind"] == "stretched" and c["facts"].J > window and len(c["read"]) == sg.N for c in cases)
            every = [c["facts"].span for j in jobs if not j["pure"] for c in j["reads"] if c["kind"] == "stretched" and c["adapter"] == job["names"][0]]
            assert max(c["facts"].span for c in cases) == max(every)
            assert min(sg.pair_bound(scheme, c["facts"].I, c["facts"].score) - c["facts"].span for c in cases) <= (-scheme[2] - g) // g
    jobs = [j for j in jobs if not j["pure"]]
    per_adapter = {}
    for c in stretched_cases(jobs):
        per_adapter.setdefault(c["adapter"], []).append(c)
    for name, cases in per_adapter.items():
        m = len(sg.ADAPTERS[name])
        assert {c["family"] for c in cases} == {"tight-pair", "widest", "truncated", "start", "start-cut"}
        copies = {(c["family"], c["L"], c["pieces"]) for c in cases if "boundary" in c}
        assert len([k for k in copies if k[0] == "tight-pair"]) == 3 and len([k for k in copies if k[0] == "widest"]) == 1
        for fam, L, pieces in copies:
            mine = [c for c in cases if (c["family"], c.get("L"), c.get("pieces")) == (fam, L, pieces)]
            span = mine[0]["facts"].span
            want = {(b, d) for b in sg.BOUNDARIES for d in (1, 2, span - m - 1, span - 1, span, span + 1)}
            assert {(c["boundary"], c["d"]) for c in mine} == want
            for c in mine:                                  # the copy ends where it was planted, and whole reads have N columns
                assert c["facts"].J == c["boundary"] + c["d"] == c["end"] and len(c["read"]) == sg.N and c["facts"].span == span
    for job in jobs:
        reads = job["reads"]
        assert len(reads) % sg.TILE == 0 and len(reads) >= 2 * sg.TILE
        for t in range(0, len(reads), sg.TILE):
            tile = reads[t:t + sg.TILE]
            assert {c["kind"] for c in tile} == set(sg.KINDS), t
            assert len({len(c["read"]) for c in tile}) >= 3
            assert sum(c["kind"] == "stretched" for c in tile) >= 50
        # the other kinds are what they are called
        m0 = len(job["ads"][0])
        for i, c in enumerate(reads):
            fields = [w[i].split(",") for w in job["want"]]
            mine = fields[[n for n in job["names"] if n].index(c["adapter"])]
            full = len(sg.ADAPTERS[c["adapter"]])
            if c["kind"] == "exact":
                assert float(mine[6]) == 100.0 and int(mine[3]) - int(mine[2]) + 1 == full
            elif c["kind"] == "nohit":
                assert not any(a[k:k + 12] in c["read"] for a in job["ads"] for k in range(len(a) - 11))   # no 12 bases of an adapter
            elif c["kind"] == "early":
                assert int(mine[1]) + 1 <= full and float(mine[5]) == 100.0
        assert len(job["want"]) == len(job["ads"]) and all(len(w) == len(reads) for w in job["want"])
        assert m0 >= len(job["ads"][-1])
