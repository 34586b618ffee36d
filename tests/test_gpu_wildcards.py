"""IUPAC wildcards in adapters on the GPU: every record bit for bit that of tests/wild_ref.py (the independent restatement of
the rule), no tolerance, no pair left out.

A wildcard context uploads its adapters as sets (pc_letters.h).  trace16_kernel builds its substitution table from them,
scan_kernel runs its wildcard variant (traced and score-only, register and LDS-state forms), the plain-int32 kernel
(pc_slow.hip) and the path kernels (pc_paths.hip) ask matches(); the specialised score kernels tell letters apart by set and
are declined only where the letter pairs outgrow the register plan.  The context settings below (packed-fp16 traced, packed-int16, the
plain-int32 schemes) choose among them.

Anchor 2 (independent of wild_ref): for an aligned pair, the concrete adapter read off the returned path -- the read's base at
a degenerate row under '=', the first member of the row's set elsewhere -- scores the same under the UNCHANGED oracle: no
concrete adapter can score higher than the wildcard alignment."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import wild_ref, wild_runner_case, wildgen

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (3, -6, -5, -2)
INT32_SCHEMES = {"affine": (3000, -6000, -5000, -2000), "linear": (3000, -6000, -4000, -4000)}     # tests/test_gpu_one_cell.py
LETTERS = "ACGTURYSWKMBDHVN"


def make(adapters, scores=DEFAULT, wildcards=True, int16=False):
    import porechop_amd
    al = porechop_amd.Aligner(adapters, scores, wildcards=wildcards)
    if int16:
        al.set_int16_only(True)
    return al


def expect(pairs, adapters, scores=DEFAULT, wildcards=True):
    return wild_ref.align_many([(rd, adapters[ai]) for rd, ai in pairs], scores, wildcards=wildcards)


def check_paths(pairs, adapters, scores, recs, heads, ops, oracle=None):
    """Test 5 for one batch: the path re-scored under the rule reproduces its record, '=' sits only on matches, and anchor 2."""
    from porechop_amd.batch import cigar
    ma, mi, go, ge = scores
    aligned = 0
    for (rd, ai), rec, hd, op in zip(pairs, recs, heads, ops):
        ad = adapters[ai]
        if rec[0] == -1:
            continue
        path = (int(hd[1]), int(hd[2]), cigar(op))
        matches, diag, gaps, ok = wild_ref.rescore(rd, ad, path, wildcards=True)
        assert ok, (rd, ad, path)
        opens = int(hd[3])
        assert ma * matches + mi * (diag - matches) + (go * opens + ge * (gaps - opens) if go != ge else ge * gaps) == rec[4], (rd, ad, path, rec)
        assert matches == rec[5]
        if oracle is None or not len(op):
            continue
        # anchor 2
        concrete = [wild_ref.first_member(ord(c)) or "N" for c in ad]
        rb, ab = path[0], path[1]
        for o in op:
            if o in "=X":
                if o == "=" and wild_ref.letter_set(ord(ad[ab]), True) != wild_ref.letter_set(ord(ad[ab]), False):
                    concrete[ab] = rd[rb].upper().replace("U", "T")
                rb += 1
                ab += 1
            elif o == "I":
                rb += 1
            else:
                ab += 1
        # (a letter of the EMPTY set has no concrete base: 'N' would match a read N under the oracle.  Only adapters with a junk
        # byte have one; those pairs are left to wild_ref and are not counted)
        if "N" in concrete:
            assert any(wild_ref.letter_set(ord(c), True) == 0 for c in ad)
            continue
        want = int(oracle.adapter_alignment(rd, "".join(concrete), scores).split(",")[4])
        assert want == rec[4], (rd, ad, "".join(concrete), want, rec)
        aligned += 1
    return aligned


def letter_panel():
    return ["ACGT" + ch + "TGCA" for ch in LETTERS + LETTERS.lower() + "@"]


def letter_windows():
    return ["GGACGT" + b + "TGCAGG" for b in wildgen.WINDOW_BYTES]


@pytest.mark.parametrize("family", ["fp16", "int16", "int32_affine", "int32_linear"])
def test_every_letter_in_every_context(family, oracle):
    adapters = letter_panel() + ["ACGTATGCA"]                     # (the last: an adapter of bases, on the family's own kernel)
    pairs = [(w, ai) for ai in range(len(adapters)) for w in letter_windows()]
    scores = INT32_SCHEMES[family[6:]] if family.startswith("int32") else DEFAULT
    want, want_paths = expect(pairs, adapters, scores)
    al = make(adapters, scores, int16=family == "int16")
    try:
        got = al.align_pairs(pairs)
        assert np.array_equal(got, want), [(pairs[k], got[k], want[k]) for k in np.nonzero((got != want).any(axis=1))[0][:5]]
        recs, heads, ops = al.align_pairs_paths(pairs)
        assert np.array_equal(recs, want)
        from porechop_amd.batch import cigar
        assert [(int(h[1]), int(h[2]), cigar(o)) for h, o in zip(heads, ops)] == want_paths
        # every pair aligns (all share ACGT / TGCA with their window); only the junk-byte adapter's 12 pairs have no concrete twin
        assert check_paths(pairs, adapters, scores, recs, heads, ops, oracle) == len(pairs) - len(letter_windows())
    finally:
        al.close()


def test_long_degenerate_adapters_on_the_plain_int32_kernel():
    """Adapters of 130 and 200 letters (above the packed kernels' 128 rows; the 200-row one keeps its column state in HBM)."""
    rng = random.Random(77)
    adapters = [wildgen.random_adapter(rng, 130, 0.3), wildgen.random_adapter(rng, 200, 0.3).upper()]
    pairs = []
    for ai, ad in enumerate(adapters):
        for where in ("start", "middle", "end", None) * 4:
            pairs.append((wildgen.read_with(rng, 300, ad, where, edits=rng.randrange(0, 12), noise=0.02), ai))
        pairs += [(wildgen.random_bases(rng, n), ai) for n in (1, 129, 130, 131, 199, 200, 201)]
    want, _ = expect(pairs, adapters)
    al = make(adapters)
    try:
        got = al.align_pairs(pairs)
        assert np.array_equal(got, want), [(got[k], want[k]) for k in np.nonzero((got != want).any(axis=1))[0][:5]]
    finally:
        al.close()


def whole_read_case(rng):
    adapters = [wildgen.UMI28, wildgen.PRIMER22, "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"]
    pairs = []
    for n in (300, 301, 777, 1500, 3000):
        for where in ("start", "middle", "end", None):
            for ai in range(len(adapters)):
                pairs.append((wildgen.read_with(rng, n, adapters[ai], where, edits=rng.randrange(0, 4), noise=0.01), ai))
    return adapters, pairs


def test_whole_reads_with_planted_degenerate_adapters(oracle):
    """Reads of 300 to 3 000 bases with planted, mutated instances of the degenerate 28-mer and 22-mer (middle, both ends, none)
    under PC_MODE_AUTO, beside adapters of bases on the two-pass packed kernels in the same call."""
    adapters, pairs = whole_read_case(random.Random(31))
    want, _ = expect(pairs, adapters)
    al = make(adapters)
    try:
        got = al.align_pairs(pairs)
        assert np.array_equal(got, want), [(pairs[k][1], got[k], want[k]) for k in np.nonzero((got != want).any(axis=1))[0][:5]]
        short = [p for p in pairs if len(p[0]) <= 777]
        recs, heads, ops = al.align_pairs_paths(short)
        assert check_paths(short, adapters, DEFAULT, recs, heads, ops, oracle) == sum(1 for o in ops if len(o))
    finally:
        al.close()


def device_job(pairs_windows):
    dev = torch.device("cuda")
    raw = "".join(pairs_windows)
    arena = torch.from_numpy(np.frombuffer((raw + "N" * 64).encode(), dtype=np.uint8).copy()).to(dev)
    lens = np.array([len(w) for w in pairs_windows], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    return arena, torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)


def scan(al, windows, ads, mode, floors=None):
    """One scan_device call: one job over `windows` with one adapter or a dual pair -> records [len(ads) * n, 8]."""
    arena, off, ln = device_job(windows)
    n = len(windows)
    out = torch.zeros((n * len(ads), 8), dtype=torch.int32, device=arena.device)
    al.scan_device(arena, off, ln, [ads[0]], [0, n], max(len(w) for w in windows), out, mode,
                   job_adapter_b=[ads[1]] if len(ads) == 2 else None, floors=None if floors is None else [floors[0]],
                   floors_b=None if floors is None or len(ads) < 2 else [floors[1]])
    al.sync()
    return out.cpu().numpy()


def edge_adapter(rng, m):
    """m letters with degenerate ones on the first row (next to the padding rows of a padded class), the last and two inside."""
    ad = [rng.choice("ACGT") for _ in range(m)]
    ad[0] = rng.choice("RYSWKMBDHVN")
    ad[-1] = rng.choice("RYSWKMBDHVN")
    for k in (m // 3, 2 * m // 3):
        ad[k] = rng.choice("RYKMBDHVNn")
    return "".join(ad)


# job (adapter lengths) -> (rows, padded) of the register class it must run alone: 5 -> 16 rows (the lowest class, eleven padding
# rows), 28 -> 28 exact, 27 -> 28 padded (three waves), 37 / 38 -> 38 (constants in registers), 41 .. 48 -> 48 (constants by LDS
# read), 75 / 100 -> 112 (above 72 rows).  Dual jobs: halves of different lengths in ONE class, and two whose halves would take
# different classes alone.  What build_table makes of each call is asked of tests/host/plan_probe.cpp below, not believed.
ROW_CLASS_JOBS = {(5,): (16, True), (28,): (28, False), (27,): (28, True), (37,): (38, True), (41,): (48, True), (100,): (112, True),
                  (28, 27): (28, True), (38, 37): (38, True), (48, 41): (48, True), (100, 75): (112, True), (16, 5): (16, True),
                  (28, 22): (28, True), (44, 37): (48, True)}
ROW_CLASS_WINDOWS = 70


@pytest.fixture(scope="module")
def probe():
    from tests import rowclassgen
    return rowclassgen.Probe(sanitize=False)


def probed_group(probe, scores, lengths, mode, int16, max_len):
    """The one group pcn::build_table makes of the job's call, as tests/host/plan_probe.cpp answers."""
    call = probe.calls(scores, [(mode, max_len, [(lengths[0], lengths[1] if len(lengths) > 1 else -1, ROW_CLASS_WINDOWS)])], int16_only=int16)[0]
    assert len(call.groups) == 1 and call.slow_jobs == 0 and call.total == ROW_CLASS_WINDOWS * len(lengths), call
    return call.groups[0]


@pytest.mark.parametrize("lengths", list(ROW_CLASS_JOBS), ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("scheme", ["affine", "linear"])
def test_row_classes_at_their_edges(lengths, scheme, probe):
    """One call per job, so the class's own kernel runs: single tiles and dual tiles whose halves differ in length (padding rows
    on one half), windows of 1, m - 1, m, m + 1, 149 and 150 columns, both lane types, traced (PC_MODE_TRACE) and score-only
    (PC_MODE_SCORE); the linear scheme takes scan_kernel's LDS-state variant.  Before each launch the plan probe must answer
    with ONE group of the stated class -- rows and padding; one tile for a single job, two for a job that stays dual; the
    packed-fp16 traced kernel exactly where the lane setting and the class have one.  Records and end cells are wild_ref's."""
    from porechop_amd.batch import MODE_SCORE, MODE_TRACE
    rng = random.Random(hash(lengths) & 0xFFFF)
    scores = DEFAULT if scheme == "affine" else (3, -6, -4, -4)
    adapters = [edge_adapter(rng, m) for m in lengths]
    m = lengths[0]
    windows = []
    for n in sorted({1, max(1, m - 1), m, m + 1, 149, 150}):
        for where in ("start", "end", "middle", None):
            windows.append(wildgen.read_with(rng, n, adapters[rng.randrange(len(adapters))], where, edits=rng.randrange(0, 3), noise=0.03)[:n].ljust(n, "A"))
    windows += [wildgen.random_bases(rng, 150, 0.1) for _ in range(ROW_CLASS_WINDOWS - len(windows))]      # more than 64
    assert len(windows) == ROW_CLASS_WINDOWS
    rows, pad = ROW_CLASS_JOBS[lengths] if scheme == "affine" else (0, True)               # linear: the LDS-state variant
    pairs = [(w, ai) for ai in range(len(adapters)) for w in windows]
    cells = []
    want, _ = wild_ref.align_many([(w, adapters[ai]) for w, ai in pairs], scores, wildcards=True, cells=cells)
    want_score = np.array([[-2, c[0], c[1], 0, r[4], 0, 0, 0] for c, r in zip(cells, want)], dtype=np.int32)
    al = make(adapters, scores)
    try:
        for int16 in (False, True):
            al.set_int16_only(int16)
            for mode in (MODE_TRACE, MODE_SCORE):
                g = probed_group(probe, scores, lengths, mode, int16, 150)
                assert (g.rows, g.pad, g.tiles) == (rows, pad, len(lengths)), (mode, int16, g)
                assert g.two_pass == (mode == MODE_SCORE)
                if mode == MODE_TRACE:
                    assert g.trace16 == (not int16 and rows in probe.trace16), (int16, g)
            got = scan(al, windows, list(range(len(adapters))), MODE_TRACE)
            assert np.array_equal(got, want), (int16, [(pairs[k], got[k], want[k]) for k in np.nonzero((got != want).any(axis=1))[0][:3]])
            got = scan(al, windows, list(range(len(adapters))), MODE_SCORE)
            assert np.array_equal(got, want_score), (int16, [(pairs[k], got[k], want_score[k]) for k in np.nonzero((got != want_score).any(axis=1))[0][:3]])
    finally:
        al.close()


def test_scheme_beyond_the_wildcard_compare_keeps_every_adapter_exact():
    """match - mismatch = 2100 is within the packed kernels' range (pc_scores_supported) and beyond what scan_kernel's wildcard
    compare holds (2^11): the wildcard variants must not be launched at all.  Gaps cost more than a mismatch and seven matches
    pay for one, so paths do cross mismatch columns -- a compare clipped at 2048 would score each 52 too high.  A panel of
    base-only adapters beside a degenerate one, wildcards on: every record is wild_ref's, and the base-only adapters' records
    are the wildcard-off context's."""
    import porechop_amd
    scores = (500, -1600, -3000, -100)
    adapters = ["ACGTACGTTAGCCA", "GGATCCTTAGCA", "ACGTNNRYTAGCCA", "TTGACCGTAACA"]
    assert porechop_amd.load_library().pc_scores_supported(*scores, max(len(a) for a in adapters)) == 1
    rng = random.Random(2101)
    pairs = []
    for ai, ad in enumerate(adapters):
        for n in (150, 149, 40, 600):
            for where in ("start", "middle", "end", None):
                for edits in (0, 1, 1, 2):
                    pairs.append((wildgen.read_with(rng, n, ad, where, edits=edits, noise=0.02), ai))
    want, _ = expect(pairs, adapters, scores)
    for int16 in (False, True):
        on, off = make(adapters, scores, int16=int16), make(adapters, scores, wildcards=False, int16=int16)
        try:
            got, plain = on.align_pairs(pairs), off.align_pairs(pairs)
            assert np.array_equal(got, want), (int16, [(pairs[k][1], got[k], want[k]) for k in np.nonzero((got != want).any(axis=1))[0][:5]])
            bases = np.array([ai != 2 for _, ai in pairs])
            assert np.array_equal(got[bases], plain[bases]), int16
            assert ((want[:, 5] < want[:, 6]) & (want[:, 4] > 0))[bases].sum() >= 10      # paths with mismatch columns among them
        finally:
            on.close()
            off.close()


def test_floored_two_pass_scan_at_a_90_percent_floor():
    """pc_scan_device_floored over whole reads, the degenerate 28-mer and 22-mer as a dual pair: pairs at or above the floor get
    the unfloored records (wild_ref's), pairs below it the "no alignment" record."""
    from porechop_amd.batch import MODE_TWO_PASS
    rng = random.Random(90)
    adapters = [wildgen.UMI28, wildgen.PRIMER22]
    reads = [wildgen.read_with(rng, n, adapters[k % 2], where, edits=rng.randrange(0, 3), noise=0.01)
             for k, (n, where) in enumerate([(n, w) for n in (300, 900, 3000) for w in ("start", "middle", "end", None) for _ in range(6)])]
    # the floor of pipeline.identity_score_bound at 90 %: m * (t * match - max penalty * (1 - t)), t = (90 - 1e-6) / 100
    t = (90.0 - 1e-6) / 100.0
    floors = [int(np.floor(len(a) * (t * 3 - 6 * (1.0 - t)))) for a in adapters]
    pairs = [(r, ai) for ai in range(2) for r in reads]
    want, _ = expect(pairs, adapters)
    al = make(adapters)
    try:
        plain = scan(al, reads, [0, 1], MODE_TWO_PASS)
        assert np.array_equal(plain, want)
        got = scan(al, reads, [0, 1], MODE_TWO_PASS, floors=floors)
        above = np.array([want[k][4] >= floors[pairs[k][1]] for k in range(len(pairs))])
        assert above.sum() >= 20 and (~above).sum() >= 20
        assert np.array_equal(got[above], want[above])
        assert (got[~above] == np.array([-1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)).all()
    finally:
        al.close()


def test_specialised_and_generic_score_kernels_in_one_child_process(tmp_path):
    """tests/wild_spec_child.py: whole reads under PC_MODE_TWO_PASS / PC_MODE_SCORE and a floored call, once over the generic
    score kernel and once over the specialised ones compiled for the degenerate pairs (one with >= 12 distinct letters per
    adapter); every record wild_ref's."""
    env = dict(os.environ, PC_JIT_MIN_CELLS="1", PC_JIT_CACHE_DIR=str(tmp_path / "jit"), PC_QUIET="1")
    env.pop("PC_DISABLE_JIT", None)
    p = subprocess.run([sys.executable, "-m", "tests.wild_spec_child"], capture_output=True, text=True, cwd=REPO, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "wild_spec_child ok compiled=" in p.stdout


def test_masked_stretch_is_no_second_hit():
    """A read whose first hit is masked with '-' under an N-rich adapter: without wildcards the '-' bytes (Dna5 code 4) equal the
    adapter's N rows; with wildcards they match nothing -- in a scan, in align_paths and in middle_paths, which masks by itself."""
    from porechop_amd.batch import cigar
    rng = random.Random(9)
    adapter = "ACGTACNNNNNNNNGTCAGT"
    body = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    read = body(400) + "ACGTAC" + body(8) + "GTCAGT" + body(400)
    stretch = "-" * 20
    dev = torch.device("cuda")
    on, off = make([adapter], wildcards=True), make([adapter], wildcards=False)
    try:
        first = on.align_pairs([(read, 0)])[0]
        assert (int(first[0]), int(first[1]), int(first[5])) == (400, 419, 20)
        masked = read[:400] + stretch + read[420:]
        pairs = [(masked, 0), (stretch, 0)]
        want, want_paths = expect(pairs, [adapter])
        recs, heads, ops = on.align_pairs_paths(pairs)
        assert np.array_equal(recs, want) and np.array_equal(on.align_pairs(pairs), want)
        assert [(int(h[1]), int(h[2]), cigar(o)) for h, o in zip(heads, ops)] == want_paths
        assert recs[1][5] == 0 and "=" not in ops[1]                   # the masked stretch alone: no match at all
        rb = int(heads[0][1])                                          # and in the whole masked read no '=' sits on a masked column
        for o in ops[0]:
            assert not (o == "=" and 400 <= rb < 420)
            rb += o in "=XI"
        recs_off, _, ops_off = off.align_pairs_paths(pairs)
        assert recs_off[1][5] == 8 and ops_off[1].count("=") == 8      # without wildcards: '-' == N on the eight N rows
        # middle_paths masks by itself: hit 1 of the read sees hit 0's interval [400, 420) as '-'
        arena = torch.from_numpy(np.frombuffer((read + "N" * 64).encode(), dtype=np.uint8).copy()).to(dev)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
        for al, matches in ((on, 0), (off, 8)):
            r2, h2, o2 = al.middle_paths(arena, t([0, 400], torch.int64), t([len(read), 20], torch.int32), t([0, 0], torch.int32),
                                         t([420, 20], torch.int32), t([0, 1], torch.int64), t([0, 1], torch.int32),
                                         t([[400, 420], [0, 20]], torch.int32))
            al.sync()
            r2 = r2.cpu().numpy()
            if al is on:
                assert np.array_equal(r2[0], first)                    # (off, the read holds no hit to take a window from)
            assert r2[1][5] == matches                                 # the stretch as its own read, masked by the interval table
    finally:
        on.close()
        off.close()


def test_adapters_of_bases_give_the_same_records_in_both_modes():
    """Consequence (i) over tests/pairgen cases, in every kernel family; and consequence (ii)."""
    from tests.pairgen import case_stream
    cases = [(rd, ad) for rd, ad in case_stream(4242, 600) if ad and not set(ad.upper()) - set("ACGTU")][:400]
    adapters = sorted({ad for _, ad in cases}, key=lambda a: (len(a), a))
    index = {a: k for k, a in enumerate(adapters)}
    pairs = [(rd, index[ad]) for rd, ad in cases]
    assert any(set(rd.upper()) - set("ACGTU") for rd, _ in pairs)
    for scores, int16 in ((DEFAULT, False), (DEFAULT, True), (INT32_SCHEMES["affine"], False), (INT32_SCHEMES["linear"], False)):
        off, on = make(adapters, scores, wildcards=False, int16=int16), make(adapters, scores, wildcards=True, int16=int16)
        try:
            a, b = off.align_pairs(pairs), on.align_pairs(pairs)
            assert np.array_equal(a, b), (scores, int16)
        finally:
            off.close()
            on.close()
    off, on = make(["NNNN"], wildcards=False), make(["NNNN"], wildcards=True)
    try:
        assert off.align_pairs_paths([("NNNN", 0)])[2] == ["===="]
        recs, _, ops = on.align_pairs_paths([("NNNN", 0)])
        assert "=" not in ops[0] and recs[0][5] == 0
        assert np.array_equal(recs, wild_ref.align_many([("NNNN", "NNNN")], DEFAULT, wildcards=True)[0])
        assert on.align_pairs_paths([("ACGT", 0)])[2] == ["===="]
    finally:
        off.close()
        on.close()


def test_one_context_through_off_on_off_on():
    """One context toggled with the same panel and with a changed panel: every step equals a fresh context's records (stale
    letter sets, tile tables, the prefilter plan's key)."""
    rng = random.Random(5)
    panel_a = [wildgen.UMI28, "AATGTACTTCGTTCAGTTACGTATTGCT", wildgen.SPACER31]
    panel_b = [wildgen.PRIMER22, "GCAATACGTAACTGAACGAAGT", "ACGTNNNNACGTACGTRY"]
    def batch(panel):
        return [(wildgen.read_with(rng, n, panel[ai], where, edits=1, noise=0.02), ai)
                for n in (150, 600) for where in ("start", "middle", None) for ai in range(3) for _ in range(2)]
    pairs_a, pairs_b = batch(panel_a), batch(panel_b)
    dev = torch.device("cuda")

    def prefilter_bits(al, panel, pairs):
        raw = "".join(rd for rd, _ in pairs)
        arena = torch.from_numpy(np.frombuffer((raw + "N" * 64).encode(), dtype=np.uint8).copy()).to(dev)
        lens = np.array([len(rd) for rd, _ in pairs], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
        ks = [al.max_edits(len(a), 85.0) for a in panel]
        got = al.prefilter(arena, torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev), int(lens.max()), list(range(len(panel))), ks)
        al.sync()
        return got.cpu().numpy()

    live = make(panel_a, wildcards=False)
    try:
        for step, (wc, panel, pairs) in enumerate([(False, panel_a, pairs_a), (True, panel_a, pairs_a), (False, panel_a, pairs_a),
                                                   (True, panel_a, pairs_a), (True, panel_b, pairs_b), (False, panel_b, pairs_b),
                                                   (True, panel_b, pairs_b)]):
            live.set_wildcards(wc)
            if panel != live_panel(live):
                live.set_adapters(panel)
            fresh = make(panel, wildcards=wc)
            try:
                want, _ = expect(pairs, panel, wildcards=wc)
                got_live, got_fresh = live.align_pairs(pairs), fresh.align_pairs(pairs)
                assert np.array_equal(got_fresh, want), step
                assert np.array_equal(got_live, want), step
                assert np.array_equal(prefilter_bits(live, panel, pairs), prefilter_bits(fresh, panel, pairs)), step
            finally:
                fresh.close()
    finally:
        live.close()


def live_panel(al):
    return [a.decode() for a in al.adapters]


def test_prefilter_stays_a_proof():
    """Windows whose instance reaches the threshold only through wildcard rows (every base under a degenerate row differs from
    the first member of its set) with real edits up to exactly max_edits: no route clears the bit of a pair whose exhaustive
    wildcard alignment reaches the threshold.  Byte route, packed route (seed stage only: refuses these lists) and packed-any."""
    from porechop_amd.io import pack_reads
    rng = random.Random(808)
    threshold = 80.0
    panel = [wildgen.UMI28, wildgen.PRIMER22, wildgen.SPACER31, "AATGTACTTCGTTCAGTTACGTATTGCT"]
    al = make(panel)
    try:
        ks = [al.max_edits(len(a), threshold) for a in panel]
        reads = []
        for ai, ad in enumerate(panel):
            for edits in range(0, ks[ai] + 1):
                for _ in range(6):
                    reads.append(wildgen.read_with(rng, 400, ad, rng.choice(["start", "middle", "end"]), edits=edits, avoid_first=True))
        reads += [wildgen.random_bases(rng, 400) for _ in range(40)]
        pairs = [(rd, ai) for rd in reads for ai in range(len(panel))]
        rec = al.align_pairs(pairs).reshape(len(reads), len(panel), 8)
        want, _ = expect(pairs, panel)
        assert np.array_equal(rec.reshape(-1, 8), want)
        hit = (rec[:, :, 0] >= 0) & (100.0 * rec[:, :, 5] >= (threshold - 1e-6) * np.maximum(rec[:, :, 7], 1))
        assert hit[:, :3].sum() >= 18                                 # at least the unedited instances
        dev = torch.device("cuda")
        arr = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
        lens = np.array([len(r) for r in reads], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
        t_off, t_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
        arena = torch.from_numpy(np.concatenate([arr, np.full(64, ord("N"), np.uint8)])).to(dev)
        pk, _ = pack_reads(arr)
        plane = torch.zeros(pk.size + 64, dtype=torch.uint8, device=dev)
        plane[:pk.size] = torch.from_numpy(pk).to(dev)
        ids = list(range(len(panel)))

        def dense(rows_bits):
            rows, bits = rows_bits
            out = np.zeros((len(reads), len(panel)), dtype=bool)
            out[rows.cpu().numpy()] = bits.cpu().numpy()
            return out

        by_bytes = dense(al.prefilter_rows(arena, t_off, t_len, 400, ids, ks))
        assert not (hit & ~by_bytes).any()
        assert (~by_bytes).sum() > 40                                 # and it does exclude: the random reads
        any_route = dense(al.prefilter_rows(plane, t_off, t_len, 400, ids, ks, packed=True, total=True))
        assert not (hit & ~any_route).any()
        assert al.prefilter_rows(plane, t_off, t_len, 400, ids, ks, packed=True) is None      # refused: the caller scans exhaustively
        # the adapter of bases alone still takes the packed seed route, at a bound the seed stage covers (90 %: 3 edits of 28)
        alone = al.prefilter_rows(plane, t_off, t_len, 400, [3], [al.max_edits(len(panel[3]), 90.0)], packed=True)
        assert alone is not None
        kept = np.zeros(len(reads), dtype=bool)
        kept[alone[0].cpu().numpy()] = alone[1].cpu().numpy()[:, 0]
        hit90 = (rec[:, 3, 0] >= 0) & (100.0 * rec[:, 3, 5] >= (90.0 - 1e-6) * np.maximum(rec[:, 3, 7], 1))
        assert hit90.sum() >= 6 and not (hit90 & ~kept).any()
    finally:
        al.close()


def test_pipeline_takes_the_byte_route_when_the_packed_route_refuses_a_degenerate_list():
    """Packed-only reads through Pipeline.phase_c(prefilter=True) with the UMI set: the packed seed route refuses the list
    (stats: packed_route_refused), the pipeline unpacks the reads and every (read, adapter) pair goes through the byte route
    (stats: pairs_middle_prefiltered = all of them), whose table is exact under the rule; the hits are those of the scan of
    every pair without any prefilter."""
    from porechop_amd.io import pack_reads
    from porechop_amd.pipeline import DeviceReads, Pipeline, ScanParams
    rng = random.Random(12)
    body = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    reads = [body(1200) + wildgen.mutate(rng, wildgen.instance(rng, wildgen.UMI28, avoid_first=True), k % 3) + body(1200) for k in range(12)]
    reads += [body(2400) for _ in range(20)]
    arr = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    dev = torch.device("cuda")
    pk, exc = pack_reads(arr)
    zero = torch.zeros(len(reads), dtype=torch.int32, device=dev)

    def hits_of(pl, rd, prefilter):
        h = pl.phase_c(rd, zero, zero, [0], prefilter=prefilter)
        pl.aligner.sync()
        return sorted(zip(h.read.cpu().tolist(), h.adapter.cpu().tolist(), h.start.cpu().tolist(), h.end.cpu().tolist()))

    pl = Pipeline(wild_runner_case.adapter_sets(), ScanParams(wildcards=True), device=dev)
    try:
        packed = DeviceReads.packed_only(pl.aligner, torch.from_numpy(pk).to(dev), arr.size, torch.from_numpy(exc).to(dev),
                                         torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev))
        got = hits_of(pl, packed, True)
        assert pl.stats.get("packed_route_refused", 0) >= 1
        assert pl.stats["pairs_middle_prefiltered"] >= len(reads) * len(pl.middle_adapters)      # round 0: all of them (+ the mask rounds)
        as_bytes = DeviceReads(torch.from_numpy(np.concatenate([arr, np.full(64, ord("N"), np.uint8)])).to(dev),
                               torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev))
        want = hits_of(pl, as_bytes, False)
        assert got == want
        found = {h[0] for h in want if pl.middle_adapters[h[1]][1] == wildgen.UMI28}
        assert set(range(0, 12, 3)) <= found                           # at least the unedited instances are hits at 90 %
    finally:
        pl.close()


def test_runner_end_to_end(tmp_path):
    """The CPU runner case on the GPU: the output is what the hand-stated trims and split say (tests/test_wildcards_cpu.py holds
    the stand-in to the same statement); without wildcards the reads come out untrimmed."""
    from porechop_amd import runner
    reads, expected = wild_runner_case.build()
    inp = wild_runner_case.write_fastq(tmp_path / "reads.fastq", reads)
    out = str(tmp_path / "on.fastq")
    res = runner.run(inp, output=out, adapter_panel=wild_runner_case.adapter_sets(), wildcards=True)
    assert res.matching_sets == ["UMI kit"]
    assert [s for _, s in wild_runner_case.read_fastq(out)] == [p for pieces in expected for p in pieces]
    from tests.wild_aligner import WildAligner
    twin = str(tmp_path / "on_stand_in.fastq")
    runner.run(inp, output=twin, aligner=WildAligner(), adapter_panel=wild_runner_case.adapter_sets(), wildcards=True)
    assert open(out, "rb").read() == open(twin, "rb").read()                # headers and quality lines too
    out = str(tmp_path / "off.fastq")
    res = runner.run(inp, output=out, adapter_panel=wild_runner_case.adapter_sets())
    assert res.matching_sets == [] and [s for _, s in wild_runner_case.read_fastq(out)] == reads
    twin = str(tmp_path / "off_stand_in.fastq")
    runner.run(inp, output=twin, aligner=WildAligner(), adapter_panel=wild_runner_case.adapter_sets())
    assert open(out, "rb").read() == open(twin, "rb").read()


def test_custom_command_line_with_the_report(tmp_path):
    """python -m porechop_amd.custom --only_custom --wildcards with the three report options: the same output bytes, and the
    CIGAR columns are wild_ref's paths of the end windows and of the chimera's middle hit."""
    reads, expected = wild_runner_case.build()
    inp = wild_runner_case.write_fastq(tmp_path / "reads.fastq", reads)
    fa = tmp_path / "umi.fasta"
    fa.write_text(">UMI kit_start\n%s\n>UMI kit_end\n%s\n" % (wild_runner_case.START, wild_runner_case.END))
    out, rep = str(tmp_path / "cli.fastq"), str(tmp_path / "cli.tsv")
    p = subprocess.run([sys.executable, "-m", "porechop_amd.custom", "-i", inp, "-o", out, "--adapters", str(fa), "--only_custom",
                        "--wildcards", "--report", rep, "--report_paths", "--report_middle_paths", "-v", "0"],
                       capture_output=True, text=True, cwd=REPO, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [s for _, s in wild_runner_case.read_fastq(out)] == [q for pieces in expected for q in pieces]
    lines = open(rep).read().split("\n")
    cols = lines[0].lstrip("#").split("\t")
    rows = [dict(zip(cols, ln.split("\t"))) for ln in lines[1:] if ln]
    assert len(rows) == len(reads)
    _, paths = wild_ref.align_many([(r[:150], wild_runner_case.START) for r in reads] + [(r[-150:], wild_runner_case.END) for r in reads],
                                   DEFAULT, wildcards=True)
    for k, row in enumerate(rows):
        assert row["start_cigars"] == "%d|%d|%s" % paths[k], k
        assert row["end_cigars"] == "%d|%d|%s" % paths[len(reads) + k], k
    chimera = reads[-1][30:len(reads[-1]) - 24]
    _, mid = wild_ref.align_many([(chimera, wild_runner_case.START)], DEFAULT, wildcards=True)
    assert rows[-1]["middle_cigars"] == "%d|%d|%s" % mid[0]
    assert all(r["middle_cigars"] == "." for r in rows[:-1])
