"""The cases of tests/rowclassgen.py, checked on the CPU before a GPU sees them: conditions, not measurements.

tests/host/plan_probe.cpp is built under ASan + UBSan (plain C++17, no HIP) and asked what pcn::build_table makes of every
scan call of the generator: each call must launch ONE group, that of its class -- nothing merged, nothing split -- and over all
calls every class of kExactRows and kPaddedRows must be launched, by a single-adapter job and by a dual one.  The oracle alone
then shows that each (class, m) job is not degenerate: it holds a near-perfect hit, alignments that end in the last column and
in the last adapter row before it, that start at column 0 and later, and one with gaps."""
import pytest

from tests import rowclassgen as gen


@pytest.fixture(scope="module")
def probe():
    return gen.Probe(sanitize=True)


@pytest.fixture(scope="module")
def cases(probe):
    return gen.Cases(probe)


@pytest.fixture(scope="module")
def plans(probe, cases):
    """(label, job, mode) -> the probe's Call, for every scan call tests/test_gpu_row_classes.py makes under the default scheme."""
    keys, calls = [], []
    for c in cases.classes:
        cc = cases.by_label[c.label]
        for jobs, modes in ((cc.end_jobs, (gen.MODE_TRACE, gen.MODE_SCORE)), (cc.whole_jobs, (gen.MODE_TWO_PASS,))):
            for job in jobs:
                for mode in modes:
                    keys.append((c.label, job, mode))
                    calls.append((mode, job.max_len, [job.probe_job()]))
    return dict(zip(keys, probe.calls(cases.scheme, calls)))


def tiles_of(job):
    per = 64 if job.dual else 128
    return (len(job.windows) + per - 1) // per


def test_the_probe_and_the_header_name_the_same_classes(probe):
    assert (probe.exact, probe.padded, probe.trace16) == gen.header_row_lists()
    assert gen.class_labels() == [c.label for c in gen.row_classes(probe.exact, probe.padded)]
    assert set(probe.trace16) == {r for r in probe.exact + probe.padded if r <= 72}


def test_lengths_are_the_edges_of_their_classes(probe, cases):
    for c in cases.classes:
        for m in c.lengths:
            assert gen.pick_rows(probe.exact, probe.padded, m, m) == (c.rows, c.pad), (c.label, m)
        if c.pad:
            low = c.lengths[0]
            assert low == 1 or gen.pick_rows(probe.exact, probe.padded, low - 1, low - 1)[0] < c.rows, (c.label, low)
            assert c.lengths[-1] == c.rows or c.rows in probe.exact, c
        for ma, mb in c.duals:
            assert gen.pick_rows(probe.exact, probe.padded, ma, mb) == (c.rows, c.pad), (c.label, ma, mb)
    # the lengths the issue names
    by = {c.label: c.lengths for c in cases.classes}
    assert (by["16"], by["24"], by["28"], by["32"], by["22e"]) == ([1, 16], [21], [27], [31], [22])


def test_every_call_launches_one_group_of_its_own_class(cases, plans):
    """Nothing merged (one group a call, with the job's own rows and padding), nothing split (a dual job is one group of dual
    tiles: its two lengths pick the same rows), and the tiles are the job's: a full one and a partly filled one, or -- 66 whole
    reads against one adapter -- a partly filled one."""
    for (label, job, mode), call in plans.items():
        c = cases.by_label[label].cls
        where = (label, job.name, mode)
        assert call.slow_jobs == 0 and len(call.groups) == 1, (where, call)
        g = call.groups[0]
        assert (g.rows, g.pad) == (c.rows, c.pad), (where, g)
        assert g.two_pass == (mode != gen.MODE_TRACE), (where, g)
        assert g.tiles == tiles_of(job), (where, g)
        assert tiles_of(job) == (1 if mode == gen.MODE_TWO_PASS and not job.dual else 2), where     # (66 whole reads: one partly filled tile)
        assert call.total == len(job.pairs()), where
        if mode == gen.MODE_TRACE:
            assert g.cols == gen.END_COLS


def test_every_class_is_launched_alone_single_and_dual(probe, plans):
    want = {(r, False) for r in probe.exact} | {(r, True) for r in probe.padded}
    for mode in (gen.MODE_TRACE, gen.MODE_SCORE, gen.MODE_TWO_PASS):
        for dual in (False, True):
            got = {(call.groups[0].rows, call.groups[0].pad) for (_, job, md), call in plans.items() if md == mode and job.dual == dual}
            assert got == want, (mode, dual, sorted(want - got), sorted(got - want))


def test_fp16_takes_the_17_classes_at_150_columns(probe, cases, plans):
    for (label, job, mode), call in plans.items():
        g = call.groups[0]
        assert g.trace16 == (g.rows in probe.trace16), (label, job.name, mode, g)
    assert sorted({call.groups[0].rows for call in plans.values() if call.groups[0].trace16}) == probe.trace16 and len(probe.trace16) == 17
    assert sorted({call.groups[0].rows for call in plans.values() if not call.groups[0].trace16}) == [112, 128]
    for r in probe.exact + probe.padded:
        assert probe.f16(cases.scheme, r, gen.END_COLS, int16_only=True)[0] is False       # pc_set_int16_only: none


def test_each_class_length_job_is_not_degenerate(cases, oracle):
    """By the oracle alone.  The gap condition holds from m = 4 on: under (3, -6, -5, -2) a gap pays only between two runs of
    at least two matches (3 min(k1, k2) > 5); the lowest length of class 16, m = 1, cannot have one."""
    match = cases.scheme[0]
    for c in cases.classes:
        for job in cases.by_label[c.label].end_jobs:
            if job.dual:
                continue
            ad, m = cases.adapters[job.ad[0]], job.lens[0]
            res = [(oracle.align_raw(w, ad, cases.scheme), len(w)) for w in job.windows]
            res = [(r, n) for r, n in res if not r.failed]
            facts = {
                "near-perfect hit": any(r.score >= 0.8 * match * m for r, n in res),
                "ends in the last column": any(r.end_j == n for r, n in res),
                "ends in the last row before the last column": any(r.end_i == m and r.end_j < n for r, n in res),
                "starts at base 0 in column 0": any(r.adapter_start == 0 and r.read_start == 0 for r, n in res),
                "starts at base 0 in a later column": any(r.adapter_start == 0 and r.read_start > 0 for r, n in res),
                "has gaps": m < 4 or any(r.read_end - r.read_start != r.adapter_end - r.adapter_start for r, n in res),
            }
            assert all(facts.values()), (job.name, facts)


def test_whole_reads_end_where_the_second_pass_has_its_edges(cases, oracle):
    """From m = 16 on (a one-base adapter is found in a read's first columns whatever is planted): best cells before column
    m (the traced window's lead-in before column 0), mid-read, one column short of the end and in the last column."""
    match = cases.scheme[0]
    for c in cases.classes:
        for job in cases.by_label[c.label].whole_jobs:
            assert max(job.wlen) < 1000, job.name
            if job.dual or job.lens[0] < 16:
                continue
            ad, m = cases.adapters[job.ad[0]], job.lens[0]
            res = [(oracle.align_raw(w, ad, cases.scheme), len(w)) for w in job.windows]
            good = [(r, n) for r, n in res if not r.failed and r.score >= 0.8 * match * m]
            facts = {
                "before column m": any(r.end_j < m for r, n in res if not r.failed),
                "mid-read": any(m < r.end_j < n - 1 for r, n in good),
                "one column short": any(r.end_j == n - 1 for r, n in good),
                "last column": any(r.end_j == n for r, n in good),
            }
            assert all(facts.values()), (job.name, facts)


def test_which_schemes_reach_the_lds_state_kernel(probe):
    """Rows 0 = scan_kernel<0, ...>.  (3, -6, -5, -5) sends every length there.  (4, -7, -10, -140) does so up to 57 bases; a
    panel with a longer adapter is outside pcb::scores_supported and runs the plain-int32 kernel: no group at all."""
    for scheme, lengths, lds in ((gen.LDS_SCHEMES[0], gen.LDS_LENGTHS, True), (gen.LDS_SCHEMES[1], gen.LDS_LENGTHS_EPS140, True),
                                 (gen.LDS_SCHEMES[1], gen.LDS_LENGTHS, False)):
        cs = gen.LdsCases(probe, scheme, lengths)
        calls = [(mode, job.max_len, [job.probe_job()]) for jobs, mode in ((cs.end_jobs, gen.MODE_TRACE), (cs.whole_jobs, gen.MODE_TWO_PASS))
                 for job in jobs]
        for call in probe.calls(scheme, calls, longest=max(lengths)):
            if lds:
                assert call.slow_jobs == 0 and [(g.rows, g.trace16) for g in call.groups] == [(0, False)], (scheme, lengths, call)
            else:
                assert call.slow_jobs >= 1 and not call.groups, (scheme, lengths, call)


def test_the_fp16_gate_and_its_column_limits(probe):
    """pcb::f16_plan's max_cols, as the probe prints them: classes 16 .. 56 with 271 .. 124 columns under (20, -30, -25, -12),
    16 .. 32 with 66 .. 32 under (5, -4, -10, -40), larger classes refused; trace16_plan changes sides exactly there."""
    want = {gen.GATE_SCHEMES[0]: ([16, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 48, 56], 271, 124),
            gen.GATE_SCHEMES[1]: ([16, 20, 22, 24, 26, 28, 30, 32], 66, 32)}
    for scheme in gen.GATE_SCHEMES:
        gc = gen.GateCases(probe, scheme)
        rows, first, last = want[scheme]
        assert gc.rows == rows and (gc.max_cols[rows[0]], gc.max_cols[rows[-1]]) == (first, last), (scheme, gc.max_cols)
        assert [gc.max_cols[r] for r in rows] == sorted((gc.max_cols[r] for r in rows), reverse=True)
        calls = probe.calls(scheme, [(gen.MODE_TRACE, job.max_len, [job.probe_job()]) for _, _, job in gc.jobs], longest=max(rows))
        for (r, at_limit, job), call in zip(gc.jobs, calls):
            assert len(call.groups) == 1 and call.groups[0].rows == r and call.groups[0].tiles == 2, (job.name, call)
            assert call.groups[0].trace16 == at_limit and call.groups[0].max_cols == gc.max_cols[r], (job.name, call)
            assert set(job.wlen) == {gc.max_cols[r] + (0 if at_limit else 1)}
        for r in probe.trace16:
            if r not in rows:
                assert probe.f16(scheme, r, 32) == (False, 0), (scheme, r)
