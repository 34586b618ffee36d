"""Middle hits for the kernel-level tests of pc_middle_paths (TEST INFRASTRUCTURE, CPU only): seeded reads of 1 to 1 920
bases with planted adapter copies, and the hits a Python restatement of the reference's mask-and-realign loop
(nanopore_read.py:216-226) finds in them over the repository's C oracle.

Adapters of 1, 8, 9, 28, 33 and 111 bases.  Every read names the adapters its loop runs, in order; the loop keeps aligning
an adapter against the progressively masked read while the full-adapter identity reaches THRESHOLD, replaces each hit's
[read_start, read_end) by '-' and stops a read after MAX_HITS hits (a one-base adapter would otherwise hit once per
occurrence of its base).  Each hit records the masked read it was aligned against -- the expected values come from aligning
that string as a whole.  The hit list is in phase C's order: round by round over all reads, so that a read's hits interleave
with the other reads' and lie in discovery order."""
import random
from collections import namedtuple

from tests.pairgen import mutate

ADAPTER_LENGTHS = (1, 8, 9, 28, 33, 111)
THRESHOLD = 85.0
MAX_HITS = 4
LONG = 1920
# (refused: the default scheme times 1000 -- the same alignments -- leaves the packed kernels' 16-bit range: pcb::compute_bounds
# refuses it and the window is the whole read)
SCHEMES = {"default": (3, -6, -5, -2), "linear": (3, -6, -4, -4), "open_above_extend": (3, -6, -2, -5),
           "refused": (3000, -6000, -5000, -2000)}

Hit = namedtuple("Hit", "read adapter start end masked rank identity")


def adapters():
    rng = random.Random(2024)
    return ["".join(rng.choice("ACGT") for _ in range(m)) for m in ADAPTER_LENGTHS]


def plant(body, copy, at):
    """copy written over body from column `at` (0-based) on; what falls outside the read is cut off."""
    for k, ch in enumerate(copy):
        if 0 <= at + k < len(body):
            body[at + k] = ch


def reads_and_plans(ads):
    """-> [(read string, [adapter indices its loop runs, in order])]"""
    rng = random.Random(99)
    rnd = lambda n: [rng.choice("ACGT") for _ in range(n)]
    A1, A8, A9, A28, A33, A111 = range(6)
    out = []

    def add(n, plants, plan):
        body = rnd(n)
        for a, at, rate in plants:
            plant(body, mutate(rng, ads[a], rate) if rate else ads[a], at)
        out.append(("".join(body), plan))

    # the shortest reads, with the one-base adapter
    add(1, [], [A1])
    add(2, [], [A1, A8])
    add(12, [(A8, 2, 0)], [A8, A1])
    add(12, [(A9, 0, 0)], [A1, A9])
    # a hit at column 1, and hits cut by the read's end / start
    for a in (A8, A9, A28, A33, A111):
        m = len(ads[a])
        add(m + 40, [(a, 0, 0)], [a])
        add(m + 40, [(a, m + 40 - (m - max(1, m // 12)), 0)], [a])          # the last m // 12 bases hang over the read's end
        add(2 * m + 7, [(a, -max(1, m // 12), 0)], [a])                     # the first ones before its start
    # the interior of reads longer than window + W (244 columns for 28 bases, 948 for 111 under the default scheme)
    for k in range(10):
        a = (A28, A33, A111, A9, A8)[k % 5]
        at = rng.randint(1000, 1400) if k % 2 else rng.randint(300, 700)
        add(LONG - (k % 3), [(a, at, (0.0, 0.04, 0.08)[k % 3])], [a])
    # three hits in one read, the same adapter twice; copies next to each other, far apart, near both ends
    for k in range(12):
        a, b = ((A28, A33), (A33, A111), (A111, A28), (A9, A28))[k % 4]
        n = min(LONG, (LONG, 1500, 977, 700)[k % 4] + k)
        gap = (0, 1, 15, 200)[k % 4]
        p0 = rng.randint(0, 40) if k % 3 == 0 else rng.randint(150, 250)
        p1 = p0 + len(ads[a]) + gap
        p2 = n - len(ads[a]) - (rng.randint(0, 30) if k % 2 else rng.randint(100, 200))
        add(n, [(a, p0, 0.03), (b, p1, 0.03), (a, p2, 0.0)], [a, b] if k % 2 else [b, a])
    # mixed lengths, one or two mutated copies, several adapters in the plan
    for k in range(70):
        n = min(LONG, (40, 150, 151, 300, 333, 700, 1200, LONG)[k % 8] + (k % 5))
        a = (A28, A33, A8, A9, A111, A28)[k % 6]
        b = (A33, A9, A28, A111, A8, A8)[k % 6]
        plants = [(a, rng.randint(0, max(0, n - len(ads[a]))), (0.0, 0.05, 0.1)[k % 3])]
        if k % 2 and n > 250:
            plants.append((b, rng.randint(0, n - len(ads[b])), 0.04))
        add(n, plants, [a, b] if k % 3 else [b, a])
    return out


def find_hits(oracle, ads, reads, scheme):
    """The mask-and-realign loop for every read -> [Hit] in phase C's order (round by round)."""
    per_read = []
    for r, (seq, plan) in enumerate(reads):
        masked, mine = seq, []
        for a in plan:
            while len(mine) < MAX_HITS:
                res = oracle.align_raw(masked, ads[a], scheme)
                if res.failed or not res.full_len:
                    break
                identity = float("%f" % ((100.0 * res.full_matches) / res.full_len))
                if identity < THRESHOLD:
                    break
                rs, re = res.read_start, res.read_end + 1
                mine.append(Hit(r, a, rs, re, masked, len(mine), identity))
                masked = masked[:rs] + "-" * (re - rs) + masked[re:]
        per_read.append(mine)
    out = []
    for rank in range(MAX_HITS):
        out += [h[rank] for h in per_read if len(h) > rank]
    return out


class Cases:
    """reads, arena (odd byte offsets, the last read ending at the arena's last byte) and, per scheme, the hits."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.adapters = adapters()
        self.reads = reads_and_plans(self.adapters)
        rng = random.Random(5)
        chunks, self.off, pos = [], [], 0
        for k, (seq, _) in enumerate(self.reads):
            pad = "N" * (rng.randint(0, 3) * 2 + (1 if (pos % 2) == 0 else 0))      # every read starts at an odd byte
            chunks += [pad, seq]
            self.off.append(pos + len(pad))
            pos += len(pad) + len(seq)
        self.arena = "".join(chunks).encode()
        self.length = [len(seq) for seq, _ in self.reads]
        assert all(o % 2 == 1 for o in self.off) and self.off[-1] + self.length[-1] == len(self.arena)
        self._hits = {}

    def hits(self, name):
        if name not in self._hits:
            self._hits[name] = find_hits(self.oracle, self.adapters, self.reads, SCHEMES[name])
        return self._hits[name]
