"""Gap-stretched adapter copies: alignments that REACH the bounds of the two-pass scan (TEST INFRASTRUCTURE, CPU only).

csrc/pc_bounds.h proves three bounds the whole-read scan relies on -- W (columns a traced path can touch left of its end
column J), the per-pair bound I + (match*I - score)/g that plan_kernel hands down as trace_cols, and SPAN (the warm-up
after which a window's values are exact).  A planted copy with a few scattered edits spans about m columns and gets near
none of them.  A copy split by a run of L filler bases does: the path crosses the run as one read gap of L columns, and
the longest run the oracle still aligns across leaves a score just above 0 (or just above what the larger piece earns
alone), i.e. a path as wide as the bounds allow.

Per (scheme, adapter) the oracle is searched for
  tight-pair   one cut in the middle, L = 1, half the largest, the largest L the oracle still aligns across;
  widest       the widest span over k = 1..6 evenly spaced pieces, both fillers, every L;
  truncated    a one-cut copy whose last 1..3 bases are cut off by the read's end (I < m), with the largest L the oracle
               still aligns across then;
  start        the largest tight-pair copy from column 1 on (J = span), and a one-cut copy whose first 1..3 bases are cut
               off by the read's start (J < span).
The tight-pair and widest copies are planted in reads of N columns so that they END at boundary + d for each of the three
chunk boundaries of a score pass cut into four chunks and d in {1, 2, span - m - 1, span - 1, span, span + 1}: the chunk
that owns J needs between none and nearly all of `span` columns of its warm-up.  Every 64 consecutive reads of a job
(a tile's worth of windows) hold stretched copies, an exact copy, a read without a hit, a hit that ends within the first
m columns and two shorter reads; the single-adapter jobs come a second time with stretched copies only (pure_jobs_for says
why).  Everything is seeded; the oracle's verdict on the finished read is what a case records."""
import random
from collections import namedtuple

from tests.longgen import Y_BOTTOM, Y_TOP

N = 1920                      # columns of a full-length read
CHUNKS = 4                    # PC_FORCE_CHUNKS the chunked routes run with
CHUNK_LEN = (N + CHUNKS - 1) // CHUNKS
BOUNDARIES = tuple(CHUNK_LEN * k for k in range(1, CHUNKS))
DEFAULT = (3, -6, -5, -2)
NO_DRIFT = (4, -7, -10, -140)
SCHEMES = (DEFAULT, (3, -6, -2, -5), (5, -4, -10, -1), (20, -30, -25, -12), (5, -4, -10, -40), NO_DRIFT, (3, -6, -5, -5), (1, -1, -1, -1))
KINDS = ("stretched", "exact", "nohit", "early", "short")
TILE = 64
FLANK = "N" * 8

Facts = namedtuple("Facts", "failed rs re a_s ae score I J span")


def no_repeat_adapter(m, seed):
    """m seeded bases, no base equal to the one before it."""
    rng = random.Random(seed)
    s = [rng.choice("ACGT")]
    while len(s) < m:
        s.append(rng.choice([c for c in "ACGT" if c != s[-1]]))
    return "".join(s)


ADAPTERS = {"Y_Top": Y_TOP, "Y_Bottom": Y_BOTTOM, "A33": no_repeat_adapter(33, 33), "A68": no_repeat_adapter(68, 68),
            "A111": no_repeat_adapter(111, 111)}


def scores_supported(scheme, m):
    """pc_bounds.h scores_supported, restated."""
    match, mismatch, go, ge = scheme
    if not (match > 0 and match > mismatch and go < 0 and ge < 0) or 6 * (match - mismatch) > 16000:
        return False
    lim = 4000 if go == ge else 8000
    return match * m <= lim and 2 * -go + m * -ge <= lim and max(-mismatch, -go, -ge) <= lim


def bounds(scheme, m):
    """pc_bounds.h compute_bounds, restated -> (W, SPAN, window, g)."""
    match, _, go, ge = scheme
    go, ge = -go, -ge
    g = min(go, ge)
    W = m + (match * m) // g
    SPAN = m + (match * m + 2 * go + (m - 1) * ge) // g + 1
    return W, SPAN, W + SPAN + 1, g


def pair_bound(scheme, I, score):
    """plan_kernel's per-pair bound, without its + 2."""
    g = min(-scheme[2], -scheme[3])
    return I + max(0, scheme[0] * I - score) // g


def adapter_names(scheme):
    """The adapters a scheme is run with: the 111-mer under the default scheme only; an adapter the scheme's values leave the
    packed kernels' range with (the 68-mer under the no-drift scheme: 2*10 + 68*140 > 8000) would run the plain-int32
    kernel, which has none of the bounds."""
    names = ["Y_Top", "Y_Bottom", "A33", "A68"] + (["A111"] if scheme == DEFAULT else [])
    return [n for n in names if scores_supported(scheme, len(ADAPTERS[n]))]


def jobs_for(scheme):
    """[(adapter A, adapter B or None)]: the panel's pair as one dual job (tiles of 64 windows, one read stream per lane, the
    longer adapter first as the built kernel cache has it), the others alone (tiles of 128 windows)."""
    names = adapter_names(scheme)
    return [("Y_Top", "Y_Bottom")] + [(n, None) for n in names if n not in ("Y_Top", "Y_Bottom")]


def pure_jobs_for(scheme):
    """The single-adapter jobs once more, as jobs of their own that hold NOTHING but stretched copies ending beyond the
    second chunk boundary (J >= 961 > window: every pass-2 window of the tile has the full length).  The columns a tile
    leaves untraced are the minimum over its pairs (notrace_upto): in a mixed tile that minimum comes from a pair with a
    loose bound of its own -- a read without a hit has the adapter-wide W + 2, a hit within the first m columns has a
    window shorter than W and switches the untraced stretch off for the whole tile -- so only a tile of stretched pairs
    alone runs with as few traced columns as its widest path needs."""
    return [j for j in jobs_for(scheme) if j[1] is None]


def cuts_for(m, k):
    return [round(i * m / k) for i in range(1, k)]


def fill(before, after, L, filler=None):
    """L filler bases between `before` and `after`: 'N's, or two bases in turn that are neither -- each filler differs from
    both of its neighbours, so none extends a match."""
    if filler == "N":
        return "N" * L
    x, y = [c for c in "ACGT" if c not in (before, after)][:2]
    return "".join((x, y)[i & 1] for i in range(L))


def stretched(adapter, cuts, L, filler=None):
    """The adapter with a run of L filler bases after each cut (a cut c splits adapter[:c] | adapter[c:])."""
    out, prev = [], 0
    for c in cuts:
        out += [adapter[prev:c], fill(adapter[c - 1], adapter[c], L, filler)]
        prev = c
    return "".join(out + [adapter[prev:]])


def facts(oracle, read, adapter, scheme):
    r = oracle.align_raw(read, adapter, scheme)
    span = 0 if r.failed else r.read_end - r.read_start + 1
    return Facts(bool(r.failed), r.read_start, r.read_end, r.adapter_start, r.adapter_end, r.score, r.end_i, r.end_j, span)


def covers(f, m):
    """The alignment covers adapter rows 0..I-1 and is wider than the adapter (not a degenerate hit with I = 1)."""
    return not f.failed and f.a_s == 0 and f.ae == f.I - 1 and f.span > m


def crossing(oracle, scheme, adapter, copy):
    """The oracle's facts for the copy between 'N' flanks if its alignment runs from the copy's first to its last base
    over every adapter row, else None."""
    f = facts(oracle, FLANK + copy + FLANK, adapter, scheme)
    m = len(adapter)
    if covers(f, m) and f.I == m and f.rs == len(FLANK) and f.span == len(copy):
        return f
    return None


def search(oracle, scheme, adapter):
    """-> {"tight": [(cuts, L, filler)] x 3, "widest": (cuts, L, filler), "crossing": every L the one-cut copy is aligned across}"""
    m = len(adapter)
    W = bounds(scheme, m)[0]
    cut = cuts_for(m, 2)
    ok = [L for L in range(1, W - m + 3) if crossing(oracle, scheme, adapter, stretched(adapter, cut, L))]
    assert ok, (scheme, m)
    tight = sorted({ok[0], ok[len(ok) // 2], ok[-1]})
    best = (m + ok[-1], cut, ok[-1], None)
    for k in range(2, 7):
        cuts = cuts_for(m, k)
        for filler in (None, "N"):
            for L in range((W - m) // (k - 1) + 1, 0, -1):
                if m + (k - 1) * L <= best[0]:
                    break
                if crossing(oracle, scheme, adapter, stretched(adapter, cuts, L, filler)):
                    best = (m + (k - 1) * L, cuts, L, filler)
                    break
    return {"tight": [(cut, L, None) for L in tight], "widest": best[1:], "crossing": ok}


def random_bases(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def plant(rng, n, copy, end, masked=False):
    """n random bases (masked: 'N's) with `copy` ending in 1-based column `end` (bases of it before column 1 or behind
    column n are cut off)."""
    body = list("N" * n if masked else random_bases(rng, n))
    for k, ch in enumerate(copy):
        c = end - len(copy) + k
        if 0 <= c < n:
            body[c] = ch
    return "".join(body)


def _case(oracle, rng, scheme, name, family, copy, end, n, want, required=True, **more):
    """A read whose oracle alignment against the adapter satisfies want(facts).  The random bases are drawn again until it
    does (a chance match beside the copy can move the alignment's first column); the widest copies score so little -- that
    is what makes them wide -- that among 1 900 random columns some chance alignment scores more: those get a read of 'N's."""
    adapter = ADAPTERS[name]
    for k in range(5):
        read = plant(rng, n, copy, end, masked=k == 4)
        f = facts(oracle, read, adapter, scheme)
        if want(f):
            d = dict(kind="stretched", family=family, adapter=name, read=read, end=end, facts=f, masked=k == 4)
            d.update(more)
            return d
    assert not required, ("no read found", scheme, name, family, end, f)
    return None


def stretched_cases(oracle, rng, scheme, name):
    adapter = ADAPTERS[name]
    m = len(adapter)
    found = search(oracle, scheme, adapter)
    out = []
    copies = [("tight-pair", c) for c in found["tight"]] + [("widest", found["widest"])]
    for family, (cuts, L, filler) in copies:
        copy = stretched(adapter, cuts, L, filler)
        span = len(copy)
        for b in BOUNDARIES:
            for d in sorted({1, 2, span - m - 1, span - 1, span, span + 1}):
                e = b + d
                out.append(_case(oracle, rng, scheme, name, family, copy, e, N,
                                 lambda f: covers(f, m) and f.I == m and f.J == e and f.span == span, boundary=b, d=d, L=L, pieces=len(cuts) + 1))
    cuts, L, filler = found["tight"][-1]
    copy = stretched(adapter, cuts, L, filler)
    span = len(copy)
    out.append(_case(oracle, rng, scheme, name, "start", copy, span, N, lambda f: covers(f, m) and f.I == m and f.J == span and f.rs == 0, L=L))

    def first(make):
        """The case of the largest L, cut by the most bases (3, 2, 1), that the oracle still aligns across the gap: the lost
        rows' matches are what the largest L's path would have paid its gap with."""
        for L in reversed(found["crossing"]):
            for t in (3, 2, 1):
                if L > t:                                   # (the span left must still exceed m)
                    c = make(stretched(adapter, cuts, L), L, t)
                    if c is not None:
                        return c
        raise AssertionError(("no cut case", scheme, name))

    out.append(first(lambda copy, L, t: _case(oracle, rng, scheme, name, "truncated", copy, N + t, N, required=False, L=L, cut=t, want=lambda f: (
        covers(f, m) and f.I == m - t and f.J == N and f.span == len(copy) - t))))
    out.append(first(lambda copy, L, t: _case(oracle, rng, scheme, name, "start-cut", copy, len(copy) - t, N, required=False, L=L, cut=t, full_span=len(copy), want=lambda f: (
        not f.failed and f.rs == 0 and f.a_s == t and f.ae == m - 1 and f.I == m and f.J == len(copy) - t))))
    return out


def other_read(rng, kind, adapter, stretched_copy):
    m = len(adapter)
    if kind == "exact":
        return plant(rng, N, adapter, rng.randint(m + 200, N - 50))
    if kind == "nohit":
        return random_bases(rng, N)
    if kind == "early":                                     # the last two thirds of the adapter from column 1 on: J <= m
        return plant(rng, N, adapter, m - m // 3)
    n = len(stretched_copy) + 5 if kind == "short" else N // 3 + rng.randint(0, 40)          # another length, a stretched copy at its end
    return plant(rng, n, stretched_copy, n - rng.randint(0, 3))


def job_reads(oracle, scheme, job, seed):
    """-> [dict(kind, adapter, read, ...)]: the stretched cases of the job's adapters, 58 to a tile of 64, the other kinds in
    the tile's last six slots; the last tile is filled up with the first cases again."""
    rng = random.Random(seed)
    names = [n for n in job if n]
    cases = []
    for n in names:
        cases += stretched_cases(oracle, rng, scheme, n)
    rng.shuffle(cases)
    per = TILE - 6
    tiles = (len(cases) + per - 1) // per
    out = []
    for t in range(tiles):
        out += [cases[(t * per + i) % len(cases)] for i in range(per)]
        name = names[t % len(names)]
        big = max((c for c in cases if c["adapter"] == name and c["family"] == "tight-pair"), key=lambda c: c["facts"].span)
        copy = big["read"][big["end"] - big["facts"].span:big["end"]]
        for kind in ("exact", "nohit", "early", "short", "short2", "exact"):
            out.append(dict(kind=kind[:5], family=None, adapter=name, read=other_read(rng, kind, ADAPTERS[name], copy)))
    return out


_memo = {}


def batch(oracle, scheme):
    """-> [dict(ads=(A, B or None) sequences, names, reads=[case dicts], want=[[the oracle's 7-field string per read] per
    adapter])] for the scheme's jobs.  Computed once per process and scheme."""
    if scheme not in _memo:
        jobs = []
        for k, job in enumerate(jobs_for(scheme)):
            reads = job_reads(oracle, scheme, job, 1000 * SCHEMES.index(scheme) + k)
            ads = [ADAPTERS[n] for n in job if n]
            want = [[oracle.adapter_alignment(c["read"], a, scheme) for c in reads] for a in ads]
            jobs.append(dict(names=job, ads=ads, reads=reads, want=want, pure=False))
        for job in pure_jobs_for(scheme):
            mixed = next(j for j in jobs if j["names"] == job)
            reads, picked = [], set()
            for i, c in enumerate(mixed["reads"]):
                if c["kind"] == "stretched" and c.get("boundary", 0) >= BOUNDARIES[1] and id(c) not in picked:
                    picked.add(id(c))
                    reads.append(i)
            jobs.append(dict(names=job, ads=mixed["ads"], reads=[mixed["reads"][i] for i in reads], want=[[w[i] for i in reads] for w in mixed["want"]],
                             pure=True))
        _memo[scheme] = jobs
    return _memo[scheme]


def tight_windows(oracle, scheme, job):
    """Windows no longer than the span: for every tight-pair and widest case of each adapter of the job, the window [first
    column of the copy, J] -> [(adapter name, [(read index, start, length)], [the oracle's string per window])]."""
    out = []
    if job["pure"]:                                         # (the same reads as the mixed job of that adapter)
        return out
    for name, ad in zip([n for n in job["names"] if n], job["ads"]):
        wins, want = [], []
        for i, c in enumerate(job["reads"]):
            if c["kind"] == "stretched" and c["adapter"] == name and c["family"] in ("tight-pair", "widest"):
                f = c["facts"]
                wins.append((i, f.rs, f.span))
                want.append(oracle.adapter_alignment(c["read"][f.rs:f.rs + f.span], ad, scheme))
        out.append((name, wins, want))
    return out
