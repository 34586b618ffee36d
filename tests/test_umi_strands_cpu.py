"""UMI groups and consensus across both strands of a molecule, without a GPU (DESIGN.md sections 17 and 18): mirror_key and
canonical on hand-stated keys, neighbours_host(strands=True) against a plain O(n^2) Levenshtein over strings, group(strands=True)
-- the ten-plus-nine case and the orientation over a chain of flips --, round_host with member_strand, the runner on the
stand-in aligner of tests/umi_aligner.py over a kit listed in both orientations with every molecule read from both strands,
the same input without umi_strands, and every new refusal."""
import random

import numpy as np
import pytest

from porechop_amd import consensus as cs
from porechop_amd import umi_groups as ug
from tests import umi_runner_case as case
from tests.umi_aligner import UmiAligner

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "V": "B", "B": "V"}


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def lev(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


# ---- the rule on keys ----------------------------------------------------------------------------------------------------------------
def test_mirror_key_and_canonical_on_stated_keys():
    assert ug.mirror_key("AAC+GGT") == "ACC+GTT"                  # rc(GGT) + rc(AAC)
    assert ug.mirror_key("ACC+GTT") == "AAC+GGT"
    assert ug.mirror_key("A+CCC") == "GGG+T"                      # the sides keep their own lengths, exchanged
    assert ug.mirror_key("aac+ggu".upper().replace("U", "T")) == "ACC+GTT"
    assert ug.bases_of(ug.mirror_key("AAC+GGT")) == rc("AACGGT")
    assert ug.canonical("AAC+GGT") == ("AAC+GGT", 0)              # AACGGT < ACCGTT
    assert ug.canonical("ACC+GTT") == ("AAC+GGT", 1)
    assert ug.canonical("TTT+TTT") == ("AAA+AAA", 1)
    assert ug.canonical("AC+GT") == ("AC+GT", 0)                  # its own mirror: a tie is strand 0
    assert ug.mirror_key("AC+GT") == "AC+GT"
    assert ug.canonical("TTN+TTT") == ("TTN+TTT", 0)              # a letter outside A C G T: its own canonical form
    assert ug.mirror_key("TTN+TTT") == "TTN+TTT"
    assert ug.canonical("+") == ("+", 0)
    with pytest.raises(ValueError):
        ug.mirror_key("ACGT")                                     # a one-sided key has no mirror


def test_mirror_planes_is_the_reverse_complement():
    rng = random.Random(5)
    keys = ["".join(rng.choice("ACGT") for _ in range(n)) for n in list(range(0, 65)) + [64, 33, 1]]
    planes, lens = ug.pack(keys)
    want, _ = ug.pack([rc(k) for k in keys])
    assert np.array_equal(ug.mirror_planes(planes, lens), want)
    garbage = planes | ~ug._len_mask(lens)[:, None]               # bits above the length are ignored
    assert np.array_equal(ug.mirror_planes(garbage, lens), want)


def _seeded_keys():
    rng = random.Random(1717)

    def mutate(s, edits):
        s = list(s)
        for _ in range(edits):
            kind = rng.randrange(3)
            if kind == 0 and s:
                s[rng.randrange(len(s))] = rng.choice("ACGT")
            elif kind == 1 and len(s) < 64:
                s.insert(rng.randrange(len(s) + 1), rng.choice("ACGT"))
            elif s:
                del s[rng.randrange(len(s))]
        return "".join(s)

    keys = []
    while len(keys) < 200:
        n = rng.choice([0, 1, 2, 8, 22, 31, 32, 33, 44, 63, 64, rng.randrange(65)])
        keys.append("".join(rng.choice("ACGT") for _ in range(n)))
    for k in range(90):                                           # planted mirrors and planted copies, 0 .. 3 edits away
        src = keys[rng.randrange(200)]
        keys.append(mutate(rc(src) if k % 3 else src, k % 4))
    # the tie: AATT is its own mirror, so d_same == d_mirror against anything; and a self-mirror key beside its neighbour
    keys += ["AATT", "AAAT", "ACGT" * 8, "ACGT" * 7 + "ACGA"]
    keys += [mutate(keys[rng.randrange(len(keys))], 1) for _ in range(300 - len(keys))]
    return keys


def test_neighbours_host_stranded_against_plain_levenshtein():
    keys = _seeded_keys()
    assert len(keys) == 300
    planes, lens = ug.pack(keys)
    mirrors = [rc(k) for k in keys]
    for max_dist in (0, 2, 3):
        want = []
        for i in range(300):
            for j in range(i + 1, 300):
                if abs(len(keys[i]) - len(keys[j])) > max_dist:
                    continue
                same, other = lev(keys[i], keys[j]), lev(keys[i], mirrors[j])
                if min(same, other) <= max_dist:
                    want.append((i, j, min(same, other), int(other < same)))
        got = ug.neighbours_host(planes, lens, max_dist, strands=True)
        assert got.dtype == np.int32 and got.shape == (len(want), 4)
        assert [tuple(r) for r in got.tolist()] == want
        if max_dist == 2:
            assert {r[3] for r in want} == {0, 1} and {r[2] for r in want} == {0, 1, 2}
            tie = [r for r in want if keys[r[0]] == "AATT" and keys[r[1]] == "AAAT"]
            assert tie == [(tie[0][0], tie[0][1], 1, 0)]                       # d_same == d_mirror == 1: flip 0
        # the unstranded call is what it was: the rows whose same-strand distance is within max_dist
        plain = ug.neighbours_host(planes, lens, max_dist)
        assert plain.shape[1] == 3
        assert [tuple(r) for r in plain.tolist()] == [(i, j, lev(keys[i], keys[j])) for i, j, _d, _f in want if lev(keys[i], keys[j]) <= max_dist]
    assert ug.neighbours_host(planes[:1], lens[:1], 2, strands=True).shape == (0, 4)


# ---- groups --------------------------------------------------------------------------------------------------------------------------
def _umis(keys):
    """RunResult.umis for reads with these START+END keys."""
    out = []
    for k in keys:
        s, e = k.split("+")
        out.append((("kit", 0, len(s), len(s), s), ("kit", 0, len(e), len(e), e)))
    return out


K_PLUS = "ACGGATCCGTAAGCTT+GGATTCAC"
K_MINUS = ug.mirror_key(K_PLUS)


def test_ten_plus_and_nine_minus_reads_are_one_group():
    assert lev(ug.bases_of(K_PLUS), ug.bases_of(K_MINUS)) > 2                  # far beyond max_dist as the keys stand
    keys = [K_PLUS] * 10 + [K_MINUS] * 9
    names = ["r%d" % k for k in range(19)]
    per_read, rows = ug.assign(_umis(keys), names, "both", 2, "directional")
    assert {g for g, _rep in per_read} == {1, 2}                  # as it stands: two molecules
    per_read, rows = ug.assign(_umis(keys), names, "both", 2, "directional", strands=True)
    canon, s = ug.canonical(K_PLUS)
    assert per_read == [(1, canon, s)] * 10 + [(1, canon, s ^ 1)] * 9
    lines = rows.splitlines()
    assert lines[0] == "r0\t1\t%s\t19\t19\t1\t%s\t%s" % (K_PLUS, canon, "+-"[s])
    assert lines[18] == "r18\t1\t%s\t19\t19\t1\t%s\t%s" % (K_MINUS, canon, "+-"[s ^ 1])
    assert ug.groups_header() == "#name\tgroup\tkey\treads_of_key\tgroup_reads\tgroup_keys\trepresentative\n"
    assert ug.groups_header(strands=True) == "#name\tgroup\tkey\treads_of_key\tgroup_reads\tgroup_keys\trepresentative\tstrand\n"
    with pytest.raises(ValueError):
        ug.assign(_umis(keys), names, "start", strands=True)


def test_a_copy_whose_error_flips_the_canonical_choice_still_joins():
    # the first base at which key and mirror differ decides the canonical form: an error there turns it over
    canon, _ = ug.canonical(K_PLUS)
    other = ug.mirror_key(canon)
    at = next(t for t in range(len(canon)) if canon[t] != other[t])
    assert canon[at] < other[at]
    noisy = canon[:at] + "T" + canon[at + 1:]                     # now above the mirror's base there (or equal to it)
    n_canon, n_s = ug.canonical(noisy)
    assert n_s == 1                                               # the noisy copy canonicalises to the other orientation
    keys = [canon] * 6 + [noisy] * 2
    per_read, _ = ug.assign(_umis(keys), ["r%d" % k for k in range(8)], "both", 2, "directional", strands=True)
    assert [p[0] for p in per_read] == [1] * 8
    assert [p[2] for p in per_read] == [0] * 8                    # mirrored to be canonical, joined over a flipped edge: + again


def test_orientation_propagates_over_a_chain_of_two_flips():
    keys, counts = ["K0", "K1", "K2", "K3"], [10, 5, 3, 1]
    pairs = np.array([[0, 1, 1, 1], [1, 2, 2, 1], [2, 3, 1, 0]])
    gid, rep, orient = ug.group(keys, counts, pairs, "directional", strands=True)
    assert gid == [1, 1, 1, 1] and rep == ["K0"] * 4 and orient == [0, 1, 0, 0]
    assert ug.group(keys, counts, pairs[:, :3], "directional") == (gid, rep)         # the walk itself is unchanged
    gid, rep, orient = ug.group(keys, [1, 1, 1, 1], pairs[::-1], "cluster", strands=True)
    assert gid == [1, 1, 1, 1] and orient == [0, 1, 0, 0]


# ---- the pile-up ---------------------------------------------------------------------------------------------------------------------
def test_round_host_reads_strand_1_as_the_reverse_complement():
    rng = random.Random(3)
    tmpl = "".join(rng.choice("ACGT") for _ in range(60))
    members = [tmpl[:20] + "A" + tmpl[20:], tmpl[:40] + tmpl[41:], tmpl[:10] + "n" + tmpl[11:], tmpl.replace("T", "U").lower()]
    stored = [rc(m.upper().replace("U", "T")) if k % 2 == 0 else m for k, m in enumerate(members)]
    strand = [1, 0, 1, 0]
    want = cs.round_host([tmpl.encode()], [m.encode() for m in members], [0] * 4, 8, 30, return_votes=True)
    got = cs.round_host([tmpl.encode()], [m.encode() for m in stored], [0] * 4, 8, 30, return_votes=True, member_strand=strand)
    assert got.cons.tobytes() == want.cons.tobytes() == tmpl.encode()
    assert np.array_equal(got.votes[0], want.votes[0]) and got.distance.tolist() == want.distance.tolist() == [1, 1, 1, 0]
    assert cs.reverse_complement_codes(cs.codes(b"ACGUNacgt")).tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3]
    assert cs.reverse_complement(b"AACG") == b"CGTT"


def test_call_groups_writes_the_plus_orientation_whatever_the_template_read():
    rng = random.Random(4)
    orig = "".join(rng.choice("ACGT") for _ in range(120))

    def sub(s, at):
        return s[:at] + "ACGT"[("ACGT".index(s[at]) + 1) % 4] + s[at + 1:]

    # five reads, all of one length: the template of round 1 is the third, a - read with an error of its own
    plus = [orig, sub(orig, 30), None, orig, sub(orig, 90)]
    seqs = [rc(sub(orig, 60)).encode() if p is None else p.encode() for p in plus]
    seqs[3] = rc(orig).encode()
    strand = [0, 0, 1, 1, 0]
    arena = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    out = cs.call_groups([(1, "K", [0, 1, 2, 3, 4])], arena, off, lens, band=8, read_strand=strand)
    assert out[0]["status"] == "called" and out[0]["sequence"] == orig.encode() and out[0]["minus"] == 2 and out[0]["used"] == 5
    assert out[0]["rounds"] == 2                                   # round 1 (in the - orientation) differs from its template read
    assert cs.fasta_text(out) == ">umi_group_1 key=K reads=5 minus=2 used=5 rounds=2 length=120\n%s\n" % orig
    assert cs.report_text(out) == ("#group\trepresentative\tmembers\tused\trejected\tskipped\trounds\tlength\tstatus\tminus\n"
                                   "1\tK\t5\t5\t0\t0\t2\t120\tcalled\t2\n")
    one = cs.call_groups([(1, "K", [0, 1, 2, 3, 4])], arena, off, lens, band=8, rounds=1, read_strand=strand)
    assert one[0]["sequence"] == orig.encode() and one[0]["rounds"] == 1
    # without the strands the two - reads are strangers to the rest
    off_ = cs.call_groups([(1, "K", [0, 1, 2, 3, 4])], arena, off, lens, band=8)
    assert "minus" not in off_[0] and off_[0]["rejected"] >= 2


# ---- the runner on the stand-in ------------------------------------------------------------------------------------------------------
KIT_REV = "UMI kit reverse"


def both_orientations():
    """The kit of tests/umi_runner_case.py and the same kit as a read of the other strand shows it: P1-UMI ... UMI-rc(P2) is
    listed as a second set whose start adapter is rc(its end adapter) and whose end adapter is rc(its start adapter)."""
    from porechop_amd.pipeline import AdapterSet
    return case.adapter_sets() + [AdapterSet(KIT_REV, ("UMI_rev_start", rc(case.END)), ("UMI_rev_end", rc(case.START)))]


MOLECULES = [("ACGACGACGACGACGA", "ACGTACGT"), ("CACACACAGAGAGAGA", "GGTTGGTT")]


def strands_case():
    """-> (records, per read (molecule, is the minus strand), the molecules' bodies).  Molecule 0: five reads, + + - - +, the
    third (the template of round 1: all are of one length) a - read with an error; molecule 1: four reads, - + - +."""
    rng = random.Random(2121)
    bodies = ["".join(rng.choice("ACGT") for _ in range(case.BODY)) for _ in MOLECULES]

    def sub(s, at):
        return s[:at] + "ACGT"[("ACGT".index(s[at]) + 1) % 4] + s[at + 1:]

    plan = [(0, 0, None), (1, 1, None), (0, 0, 50), (1, 0, None), (0, 1, 120), (1, 1, 80), (0, 1, None), (1, 0, 200), (0, 0, None)]
    records, truth = [], []
    for k, (mol, minus, err) in enumerate(plan):
        u, e = MOLECULES[mol]
        body = bodies[mol] if err is None else sub(bodies[mol], err)
        seq = case.start_instance(u) + body + case.end_instance(e)
        records.append(("read_%d" % (k + 1), rc(seq) if minus else seq))
        truth.append((mol, minus))
    return records, truth, bodies


def _run(tmp_path, tag, streamed=False, **kw):
    from porechop_amd import runner
    inp = tmp_path / "reads.fastq"
    inp.write_text(case.fastq_text(strands_case()[0]))
    out = tmp_path / ("out_%s.fastq" % tag)
    opts = runner.Options()
    opts.check_reads = 9
    if streamed:
        return runner.run_streamed(str(inp), str(out), None, opts, aligner=UmiAligner(), adapter_panel=both_orientations(), wildcards=True,
                                   **kw), out
    return runner.run(str(inp), output=str(out), options=opts, aligner=UmiAligner(), adapter_panel=both_orientations(), wildcards=True,
                      **kw), out


def test_runner_groups_and_calls_across_both_strands(tmp_path):
    records, truth, bodies = strands_case()
    groups, fa, tsv = tmp_path / "groups.tsv", tmp_path / "cons.fasta", tmp_path / "cons.tsv"
    res, out = _run(tmp_path, "on", umi=True, umi_groups=str(groups), umi_consensus=str(fa), umi_consensus_report=str(tsv), umi_strands=True)
    plus_keys = [case.start_umi(u) + "+" + e for u, e in MOLECULES]
    # every read has the key its strand shows
    lines = groups.read_text().splitlines()
    assert lines[0] == "#name\tgroup\tkey\treads_of_key\tgroup_reads\tgroup_keys\trepresentative\tstrand"
    assert len(lines) == 10
    canon = [ug.canonical(k) for k in plus_keys]
    group_of = {0: 1, 1: 2}                                       # five reads before four
    for k, (mol, minus) in enumerate(truth):
        key = ug.mirror_key(plus_keys[mol]) if minus else plus_keys[mol]
        strand = canon[mol][1] ^ minus                            # + is the orientation of the canonical key
        n = (5, 4)[mol]
        assert lines[1 + k] == "read_%d\t%d\t%s\t%d\t%d\t1\t%s\t%s" % (k + 1, group_of[mol], key, n, n, canon[mol][0], "+-"[strand])
        assert res.umi_groups[k] == (group_of[mol], canon[mol][0], strand)
    # one consensus per molecule, in the + orientation, minus= stated
    want = []
    for mol in (0, 1):
        body = bodies[mol][2:-2]
        seq = rc(body) if canon[mol][1] else body
        minus = sum(1 for m, mi in truth if m == mol and (canon[mol][1] ^ mi))
        want.append((mol + 1, canon[mol][0], (5, 4)[mol], minus, seq))
    got = res.consensus
    assert [(r["group"], r["representative"], r["members"], r["minus"], r["sequence"].decode()) for r in got] == want
    assert all(r["status"] == "called" and r["rejected"] == 0 for r in got)
    text = fa.read_text().splitlines()
    assert text[0] == ">umi_group_1 key=%s reads=5 minus=%d used=5 rounds=%d length=236" % (canon[0][0], want[0][3], got[0]["rounds"])
    assert text[1] == want[0][4] and text[3] == want[1][4]
    assert tsv.read_text().splitlines()[0].split("\t")[-2:] == ["status", "minus"]
    assert tsv.read_text().splitlines()[1].split("\t")[-1] == str(want[0][3])

    # the same input without umi_strands: the bytes of today -- two groups per molecule, seven columns, no minus
    groups0, fa0, tsv0 = tmp_path / "groups0.tsv", tmp_path / "cons0.fasta", tmp_path / "cons0.tsv"
    res0, out0 = _run(tmp_path, "off", umi=True, umi_groups=str(groups0), umi_consensus=str(fa0), umi_consensus_report=str(tsv0))
    assert out0.read_bytes() == out.read_bytes()                  # written reads are not re-oriented, headers not changed
    lines0 = groups0.read_text().splitlines()
    assert lines0[0] == ug.groups_header().rstrip("\n") and all(len(l.split("\t")) == 7 for l in lines0)
    assert len({l.split("\t")[1] for l in lines0[1:]}) == 4 and all(len(e) == 2 for e in res0.umi_groups)
    assert "minus" not in fa0.read_text() and "minus" not in tsv0.read_text() and all("minus" not in r for r in res0.consensus)
    per_read, rows = ug.assign(res0.umis, ["read_%d" % (k + 1) for k in range(9)], "both")
    assert groups0.read_text() == ug.groups_header() + rows and res0.umi_groups == per_read

    # the streamed driver carries the option for groups
    groups_s = tmp_path / "groups_s.tsv"
    res_s, _ = _run(tmp_path, "s", streamed=True, umi=True, umi_groups=str(groups_s), umi_strands=True)
    assert res_s is not None and groups_s.read_text() == groups.read_text() and res_s.umi_groups == res.umi_groups


def test_usage_errors(tmp_path):
    from porechop_amd import runner
    g, fa = tmp_path / "g.tsv", tmp_path / "c.fasta"
    with pytest.raises(runner.UsageError, match="--umi_strands needs --umi$"):
        _run(tmp_path, "e1", umi_strands=True)
    with pytest.raises(runner.UsageError, match="--umi_strands needs --umi_groups or --umi_consensus"):
        _run(tmp_path, "e2", umi=True, umi_strands=True)
    for by in ("start", "end"):
        with pytest.raises(runner.UsageError, match="--umi_strands needs --umi_group_by both"):
            _run(tmp_path, "e3", umi=True, umi_groups=str(g), umi_group_by=by, umi_strands=True)
        with pytest.raises(runner.UsageError, match="--umi_strands needs --umi_group_by both"):
            _run(tmp_path, "e4", umi=True, umi_consensus=str(fa), umi_group_by=by, umi_strands=True)
        with pytest.raises(runner.UsageError, match="--umi_strands needs --umi_group_by both"):
            _run(tmp_path, "e5", streamed=True, umi=True, umi_groups=str(g), umi_group_by=by, umi_strands=True)
    with pytest.raises(runner.UsageError, match="--umi_strands needs --umi$"):
        _run(tmp_path, "e6", streamed=True, umi_strands=True)
    with pytest.raises(runner.UsageError, match="--umi_strands needs --umi_groups"):
        _run(tmp_path, "e7", streamed=True, umi=True, umi_strands=True)
    # a panel with a UMI on one side only: no START+END key, so no mirror
    from porechop_amd.pipeline import AdapterSet
    one_side = [AdapterSet("one side", ("one_start", case.START), ("one_end", "GCTAGTCAGGTCCTGATCCATGAGTC"))]
    inp = tmp_path / "reads.fastq"
    with pytest.raises(runner.UsageError, match="--umi_strands needs degenerate letters in a start and in an end adapter"):
        runner.run(str(inp), output=str(tmp_path / "out_e8.fastq"), options=runner.Options(), aligner=UmiAligner(), adapter_panel=one_side,
                   wildcards=True, umi=True, umi_groups=str(g), umi_strands=True)
    assert not g.exists() and not fa.exists() and not list(tmp_path.glob("out_*"))
    assert "umi_strands" not in runner.Options.__dataclass_fields__


def test_command_line():
    from porechop_amd.custom import build_custom_parser
    a = build_custom_parser().parse_args(["-i", "x.fastq", "--umi", "--umi_groups", "g.tsv", "--umi_strands"])
    assert a.umi_strands is True
    assert build_custom_parser().parse_args(["-i", "x.fastq"]).umi_strands is False
    assert "--umi_strands" in build_custom_parser().format_help()
