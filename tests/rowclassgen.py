"""Cases that launch every row class of the packed DP kernels ALONE, at its edges (TEST INFRASTRUCTURE, seeded, no GPU).

The register kernels are template instantiations per row class (porechop_amd/csrc/pc_kernels.h: kExactRows, kPaddedRows,
kTrace16Rows), and pcn::build_table merges the small single-pass groups of a call into the next larger class: a test that sends
a few hundred windows per adapter length in one call runs four or five of them.  Here every job is a scan call of its own, so
its class is launched by itself, and which kernel a call launches is not believed but asked: `Probe` compiles
tests/host/plan_probe.cpp (the plan headers, host only) and answers with build_table's groups, trace16_plan and the two-pass
bounds.  tests/test_row_class_cases_cpu.py checks the cases on the CPU, tests/test_gpu_row_classes.py runs them.

Per class R: the lowest adapter length that maps to it (most padding rows) and R itself (none); per (class, m) a ragged job of
130 windows (a full 128-pair tile and a 2-pair tile) whose lengths take 1, 2, m - 1, m, m + 1, 149, 150 in turn, one job of
150-column windows, two dual jobs of 66 windows with the short adapter in the low and in the high half, and whole reads
of window(m) + 40 .. + 200 columns for the two-pass scan.
"""
import atexit
import os
import random
import re
import shutil
import subprocess
import tempfile
from collections import namedtuple

from tests.pairgen import mutate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "porechop_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
MODE_AUTO, MODE_TRACE, MODE_TWO_PASS, MODE_SCORE = 0, 1, 2, 3          # include/porechop_amd.h
DEFAULT_SCHEME = (3, -6, -5, -2)
LDS_SCHEMES = [(3, -6, -5, -5), (4, -7, -10, -140)]                   # linear gaps; a gap extension too large to drift in int16
GATE_SCHEMES = [(20, -30, -25, -12), (5, -4, -10, -40)]               # f16_plan admits windows of a few dozen to 271 columns
F16_LIMIT = 2040                                                      # pcb::kF16Limit: the integers the packed-fp16 kernel may form
ALPHABETS = ["ACGT", "ACGTN", "ACGT-", "acgtACGTUu"]
END_WINDOWS, DUAL_WINDOWS, WHOLE_READS = 130, 66, 66
END_COLS = 150


def header_row_lists():
    """(kExactRows, kPaddedRows, kTrace16Rows) as pc_kernels.h spells them: what the tests are parametrised over at collection
    time, before anything is compiled.  The probe prints the lists the compiler sees; the CPU test compares the two."""
    text = open(os.path.join(CSRC, "pc_kernels.h")).read()

    def one(name):
        return [int(x) for x in re.search(r"static const int %s\[\] = \{([^}]*)\}" % name, text).group(1).split(",")]
    return one("kExactRows"), one("kPaddedRows"), one("kTrace16Rows")


Group = namedtuple("Group", "rows pad two_pass tiles cols trace16 max_cols")
Call = namedtuple("Call", "groups slow_jobs total")


class Probe:
    """tests/host/plan_probe.cpp, compiled once (ASan + UBSan unless sanitize=False) into a directory of its own."""

    def __init__(self, sanitize=True):
        self.dir = tempfile.mkdtemp(prefix="plan_probe_")
        atexit.register(shutil.rmtree, self.dir, True)
        self.exe = os.path.join(self.dir, "plan_probe")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + (SANITIZE if sanitize else []) +
                              ["-I", CSRC, os.path.join(REPO, "tests", "host", "plan_probe.cpp"), "-o", self.exe])
        self._lists()

    @classmethod
    def at(cls, exe):
        """The probe somebody else compiled (the child process of the GPU tests takes its parent's)."""
        self = cls.__new__(cls)
        self.dir, self.exe = os.path.dirname(exe), exe
        self._lists()
        return self

    def _lists(self):
        self._bounds = {}
        head = self.ask("")
        assert [l.split()[0] for l in head] == ["exact", "padded", "trace16"], head
        self.exact, self.padded, self.trace16 = ([int(x) for x in l.split()[1:]] for l in head)

    def ask(self, text):
        res = subprocess.run([self.exe], input=text, capture_output=True, text=True, timeout=120)
        lines = res.stdout.splitlines()
        assert res.returncode == 0 and not any(l.startswith("error") for l in lines), (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
        return lines

    def answers(self, scheme, text, int16_only=False, longest=128):
        head = "scheme %d %d %d %d\nint16_only %d\nlongest %d\n" % (tuple(scheme) + (1 if int16_only else 0, longest))
        return self.ask(head + text)[3:]

    def bounds(self, scheme, m):
        """(W, SPAN, window) of pcb::compute_bounds; window 0: refused."""
        if (scheme, m) not in self._bounds:                  # (asked for all lengths at once: one process a scheme)
            for l in self.answers(scheme, "".join("bounds %d\n" % k for k in range(1, 129))):
                f = l.split()
                assert f[0] == "bounds", l
                self._bounds[(scheme, int(f[1]))] = (int(f[2]), int(f[3]), int(f[4]))
        return self._bounds[(scheme, m)]

    def f16(self, scheme, rows, cols, int16_only=False):
        """(pcn::trace16_plan(rows, cols), pcb::f16_plan(rows).max_cols or 0)."""
        f = self.answers(scheme, "f16 %d %d\n" % (rows, cols), int16_only)[0].split()
        assert f[:3] == ["f16", str(rows), str(cols)], f
        return f[3] == "1", int(f[4])

    def calls(self, scheme, calls, int16_only=False, longest=128):
        """calls: [(mode, max_len, [(m, mb or -1, windows), ...]), ...] -> one Call each, with build_table's groups."""
        text = "".join("call %d %d %d\n" % (mode, max_len, len(jobs)) + "".join("%d %d %d\n" % j for j in jobs)
                       for mode, max_len, jobs in calls)
        lines = self.answers(scheme, text, int16_only, longest)
        out, at = [], 0
        for _ in calls:
            f = lines[at].split()
            assert f[0] == "call", lines[at]
            ng = int(f[1])
            groups = []
            for l in lines[at + 1:at + 1 + ng]:
                g = l.split()
                assert g[0] == "group", l
                v = [int(x) for x in g[1:]]
                groups.append(Group(v[0], bool(v[1]), bool(v[2]), v[3], v[4], bool(v[5]), v[6]))
            out.append(Call(groups, int(f[2]), int(f[3])))
            at += 1 + ng
        assert at == len(lines), lines[at:]
        return out


# ---- the classes and their adapter lengths --------------------------------------------------------------------------

def pick_rows(exact, padded, m_lo, m_hi):
    """pck::pick_rows over the given lists -> (rows, pad); rows 0: no register variant."""
    m = max(m_lo, m_hi)
    if m_lo == m_hi and m in exact:
        return m, False
    for r in padded:
        if r >= m:
            return r, True
    return 0, True


RowClass = namedtuple("RowClass", "label rows pad lengths duals")      # duals: [(m, mb), ...]


def row_classes(exact, padded):
    """Every class with its adapter lengths: a padded class R its lowest length (the previous class + 1, unless an exact class
    takes that length) and R itself where R is no exact class; an exact class m = R.  Labels: "26", and "24e" for exact."""
    out = []
    prev = 0
    for r in padded:
        low = [m for m in range(prev + 1, r + 1) if pick_rows(exact, padded, m, m) == (r, True)]
        assert low, "no adapter length maps to the padded class %d" % r
        lengths = [low[0]] + ([r] if r not in exact and r != low[0] else [])
        # two adapters of different lengths never take an exact class: (lowest | R) and (R | lowest) are this class's
        out.append(RowClass(str(r), r, True, lengths, [(low[0], r), (r, low[0])]))
        prev = r
    for r in exact:
        out.append(RowClass("%de" % r, r, False, [r], [(r, r), (r, r)]))
    return sorted(out, key=lambda c: (c.rows, c.pad))


def class_labels():
    exact, padded, _ = header_row_lists()
    return [c.label for c in row_classes(exact, padded)]


# ---- windows --------------------------------------------------------------------------------------------------------

def random_adapter(rng, m, with_n):
    ad = [rng.choice("ACGT") for _ in range(m)]
    if with_n and m >= 4:
        ad[rng.randrange(m)] = "N"
    return "".join(ad)


def place(w, copy, end):
    """Overwrite list w so that the copy's last base sits in column end - 1; what falls off either edge is cut."""
    start = end - len(copy)
    for k, ch in enumerate(copy):
        if 0 <= start + k < len(w):
            w[start + k] = ch


PLANTS = ("at column 0", "ends in the last column", "cut by the left edge", "cut by the right edge",
          "mutated 0.05", "mutated 0.15", "mutated 0.25", "two copies", "nothing")


def plant(rng, w, ad, kind):
    n, m = len(w), len(ad)
    if kind == 0:
        place(w, ad, m)
    elif kind == 1:
        place(w, ad, n)
    elif kind == 2:
        place(w, ad, m - rng.randint(1, max(1, m // 2)))
    elif kind == 3:
        place(w, ad, n + rng.randint(1, max(1, m // 2)))
    elif kind in (4, 5, 6):
        cp = mutate(rng, ad, (0.05, 0.15, 0.25)[kind - 4])
        place(w, cp, rng.randint(min(len(cp), n), n))
    elif kind == 7:
        if n >= 2 * m + 1:                                   # two whole copies: equal scores, the earliest end cell wins
            first = rng.randint(m, n - m - 1)
            place(w, ad, first)
            place(w, ad, rng.randint(first + m, n))
        else:                                                # no room: one at either edge, overlapping
            place(w, ad, m)
            place(w, ad, n)


def special_lengths(ms):
    sp = []
    for v in (1, 2) + tuple(m + d for m in ms for d in (-1, 0, 1)) + (END_COLS - 1, END_COLS):
        if 1 <= v <= END_COLS and v not in sp:
            sp.append(v)
    return sp


class Job:
    """One scan call: `windows` against adapters[ad[0]] and, dual, also against adapters[ad[1]]; the windows lie in one
    arena with gaps of 0..3 junk bytes between them (every byte alignment) and 64 bytes behind the last."""

    def __init__(self, rng, name, ad, lens, windows, max_len):
        self.name, self.ad, self.lens, self.windows, self.max_len = name, tuple(ad), tuple(lens), windows, max_len
        parts, self.off, pos = [], [], 0
        for w in windows:
            gap = "".join(rng.choice("ACGTN") for _ in range(rng.randint(0, 3)))
            parts.append(gap + w)
            pos += len(gap)
            self.off.append(pos)
            pos += len(w)
        self.arena = ("".join(parts) + "N" * 64).encode()
        self.wlen = [len(w) for w in windows]
        assert all(self.arena[o:o + n].decode() == w for o, n, w in zip(self.off, self.wlen, windows))

    @property
    def dual(self):
        return len(self.ad) == 2

    def probe_job(self):
        return (self.lens[0], self.lens[1] if self.dual else -1, len(self.windows))

    def pairs(self):
        """(window, adapter index) in the order of the call's records: adapter A's first, then B's."""
        return [(w, a) for a in self.ad for w in self.windows]


def end_job(rng, name, ad, adapters, count, uniform=False):
    seqs = [adapters[a] for a in ad]
    sp = special_lengths([len(s) for s in seqs])
    windows = []
    for i in range(count):
        n = END_COLS if uniform else (sp[(i // 2) % len(sp)] if i % 2 == 0 else rng.randint(1, END_COLS))
        alphabet = ALPHABETS[rng.randrange(len(ALPHABETS))] if rng.random() < 0.5 else "ACGT"
        w = [rng.choice(alphabet) for _ in range(n)]
        plant(rng, w, seqs[(i // len(PLANTS)) % len(seqs)], i % len(PLANTS))
        windows.append("".join(w))
    return Job(rng, name, ad, [len(s) for s in seqs], windows, END_COLS)


def whole_job(rng, name, ad, adapters, count, window):
    """Whole reads of window + 40 .. window + 200 columns; the copies end in a column < m (the second pass's lead-in before
    column 0), mid-read, one column short of the end and in the last column."""
    seqs = [adapters[a] for a in ad]
    reads = []
    for i in range(count):
        n = window + rng.randint(40, 200)
        alphabet = ALPHABETS[rng.randrange(len(ALPHABETS))] if rng.random() < 0.3 else "ACGT"
        w = [rng.choice(alphabet) for _ in range(n)]
        s = seqs[(i // 4) % len(seqs)]
        m = len(s)
        end = (rng.randint(1, max(1, m - 1)), rng.randint(m + 1, n - 2), n - 1, n)[i % 4]
        what = (i // 8) % 6
        if what == 5:                                        # two copies
            place(w, s, rng.randint(m, max(m, n // 2)))
            place(w, s, max(end, min(n, n // 2 + m)))
        elif what != 4:                                      # (4: nothing)
            place(w, s if what < 2 else mutate(rng, s, (0.05, 0.15)[what - 2]), end)
        reads.append("".join(w))
    return Job(rng, name, ad, [len(s) for s in seqs], reads, max(len(r) for r in reads))


# ---- the cases ------------------------------------------------------------------------------------------------------

class ClassCases:
    def __init__(self, cls):
        self.cls = cls
        self.end_jobs, self.whole_jobs = [], []             # each job is a call of its own


class Cases:
    """All row classes under DEFAULT_SCHEME: .adapters (one table for one Aligner), .by_label[label] -> ClassCases."""

    def __init__(self, probe, seed=20261020):
        self.scheme = DEFAULT_SCHEME
        self.classes = row_classes(probe.exact, probe.padded)
        self.adapters, self.by_label = [], {}
        serial = 0
        for c in self.classes:
            rng = random.Random(seed * 1000 + c.rows * 2 + (1 if c.pad else 0))
            cc = self.by_label[c.label] = ClassCases(c)
            index = {}
            for m in sorted(set(c.lengths) | {m for d in c.duals for m in d}):
                index[m] = len(self.adapters)
                self.adapters.append(random_adapter(rng, m, serial % 10 == 3))
                serial += 1
            other = len(self.adapters)                       # an exact class: a second adapter of the same length
            if not c.pad:
                self.adapters.append(random_adapter(rng, c.rows, False))
            for m in c.lengths:
                cc.end_jobs.append(end_job(rng, "%s m=%d ragged" % (c.label, m), [index[m]], self.adapters, END_WINDOWS))
            cc.end_jobs.append(end_job(rng, "%s m=%d 150" % (c.label, c.lengths[-1]), [index[c.lengths[-1]]], self.adapters, END_WINDOWS, True))
            for k, (ma, mb) in enumerate(c.duals):
                ad = [index[ma], index[mb]] if c.pad else ([index[ma], other] if k == 0 else [other, index[ma]])
                cc.end_jobs.append(end_job(rng, "%s (%d | %d)%s" % (c.label, ma, mb, " swapped" if k else ""), ad, self.adapters, DUAL_WINDOWS))
            for m in c.lengths:
                cc.whole_jobs.append(whole_job(rng, "%s m=%d whole" % (c.label, m), [index[m]], self.adapters, WHOLE_READS,
                                               probe.bounds(self.scheme, m)[2]))
            for k, (ma, mb) in enumerate(c.duals):
                ad = [index[ma], index[mb]] if c.pad else ([index[ma], other] if k == 0 else [other, index[ma]])
                window = max(probe.bounds(self.scheme, ma)[2], probe.bounds(self.scheme, mb)[2])
                cc.whole_jobs.append(whole_job(rng, "%s (%d | %d) whole%s" % (c.label, ma, mb, " swapped" if k else ""), ad, self.adapters,
                                               WHOLE_READS, window))


class LdsCases:
    """The LDS-state kernel scan_kernel<0, ...>: what every scheme that cannot drift runs (pc_scan_plan.h: no_drift).  Adapter
    lengths `lengths` and the dual (lengths[0] | lengths[-1]); end windows for MODE_TRACE, whole reads for MODE_TWO_PASS."""

    def __init__(self, probe, scheme, lengths, seed=20261021):
        rng = random.Random(seed + sum(scheme) + 7 * lengths[-1])
        self.scheme, self.lengths = scheme, list(lengths)
        self.adapters = [random_adapter(rng, m, False) for m in lengths]
        self.end_jobs, self.whole_jobs = [], []
        jobs = [[i] for i in range(len(lengths))] + [[0, len(lengths) - 1], [len(lengths) - 1, 0]]
        for ad in jobs:
            name = "lds %s %s of %s" % (scheme, " | ".join(str(lengths[a]) for a in ad), self.lengths)
            self.end_jobs.append(end_job(rng, name, ad, self.adapters, END_WINDOWS if len(ad) == 1 else DUAL_WINDOWS))
            ws = [probe.bounds(scheme, lengths[a])[2] for a in ad]
            window = max(ws) if all(ws) else 2 * END_COLS    # (refused: the plain-int32 kernel takes it, over the whole read)
            self.whole_jobs.append(whole_job(rng, name + " whole", ad, self.adapters, WHOLE_READS, window))


# The lengths of the LDS-state cases.  Under (4, -7, -10, -140) pcb::scores_supported refuses a panel whose longest adapter is
# above 57 bases (2 |open| + m |extend| <= 8000): lengths 127 and 128 then leave the packed kernels altogether and run the
# plain-int32 kernel, by the probe.  They are run all the same; 56 and 57 are what reaches the LDS-state kernel at its top there.
LDS_LENGTHS = [1, 2, 127, 128]
LDS_LENGTHS_EPS140 = [1, 2, 56, 57]


class GateCases:
    """The column limit of the packed-fp16 traced kernel (pcb::f16_plan max_cols, taken from the probe): per admitted class two
    jobs of 130 windows, every window exactly max_cols and exactly max_cols + 1 columns long, against an adapter of R bases.
    The windows hold an exact copy ending in the last column (the tracked term M + R eps at full drift), a copy at column 0
    followed by junk, and homopolymer junk."""

    def __init__(self, probe, scheme, seed=20261022):
        rng = random.Random(seed + sum(scheme))
        self.scheme = scheme
        self.max_cols = {r: probe.f16(scheme, r, 1)[1] for r in probe.trace16}
        self.rows = [r for r in probe.trace16 if self.max_cols[r] > 0]
        self.adapters = [random_adapter(rng, r, False) for r in self.rows]
        self.jobs = []                                       # (rows, at the limit?, Job)
        for k, r in enumerate(self.rows):
            ad = self.adapters[k]
            for cols in (self.max_cols[r], self.max_cols[r] + 1):
                windows = []
                for i in range(END_WINDOWS):
                    if i % 3 == 2:
                        w = [rng.choice("ACGT")] * cols
                    else:
                        w = [rng.choice("ACGT") for _ in range(cols)]
                        place(w, ad, cols if i % 3 == 0 else r)
                    windows.append("".join(w))
                self.jobs.append((r, cols == self.max_cols[r], Job(rng, "gate %s R=%d cols=%d" % (scheme, r, cols), [k], [r], windows, cols)))
