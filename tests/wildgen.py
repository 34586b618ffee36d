"""TEST INFRASTRUCTURE: seeded cases for the IUPAC-wildcard tests -- degenerate adapters, concrete instances of them, reads
with planted and mutated instances.  Shared by the CPU and GPU wildcard tests; expectations come from tests/wild_ref.py."""
import random

from tests import wild_ref

UMI28 = "TTTVVVVTTVVVVTTVVVVTTVVVVTTT"            # a UMI adapter: twelve V = ACG
PRIMER22 = "GCRATACGYAACNGAACGWAGT"              # a primer with R, Y, N, W positions
SPACER31 = "AATGTACTTCGTNNNNCAGTTACGTATTGCT"     # a barcode flank with an NNNN spacer
LETTERS = "ACGTURYSWKMBDHVN"
WINDOW_BYTES = "ACGTUNacgt-X"
SCHEMES = [(3, -6, -5, -2), (3, -6, -5, -2), (2, -3, -4, -1), (5, -4, -6, -6), (3, -6, -3, -3), (1, -1, -2, -1)]


def instance(rng, adapter, avoid_first=False):
    """A concrete sequence the adapter matches base for base under the rule; a letter of the empty set gets any base.
    avoid_first: never the first member of a set of several -- an instance that reaches a threshold through its wildcard rows
    only."""
    out = []
    for ch in adapter:
        s = wild_ref.letter_set(ord(ch), True)
        members = [b for k, b in enumerate("ACGT") if s >> k & 1] or list("ACGT")
        if avoid_first and len(members) > 1:
            members = members[1:]
        out.append(rng.choice(members))
    return "".join(out)


def mutate(rng, s, edits):
    s = list(s)
    for _ in range(edits):
        k = rng.randrange(len(s)) if s else 0
        kind = rng.randrange(3)
        if kind == 0 and s:
            s[k] = rng.choice([b for b in "ACGT" if b != s[k]])
        elif kind == 1 and s:
            del s[k]
        else:
            s.insert(k, rng.choice("ACGT"))
    return "".join(s)


def random_bases(rng, n, noise=0.0):
    return "".join(rng.choice("Nn-acgtX") if rng.random() < noise else rng.choice("ACGT") for _ in range(n))


def read_with(rng, n, adapter, where, edits=0, noise=0.0, avoid_first=False):
    """n random bases with one (mutated) instance of `adapter` at the start, the end or in the middle; where None: none."""
    if where is None:
        return random_bases(rng, n, noise)
    inst = mutate(rng, instance(rng, adapter, avoid_first), edits)
    rest = max(0, n - len(inst))
    left = {"start": rng.randrange(0, 4), "end": max(0, rest - rng.randrange(0, 4)), "middle": rest // 2 + rng.randrange(-5, 6)}[where]
    left = min(max(left, 0), rest)
    return random_bases(rng, left, noise) + inst + random_bases(rng, rest - left, noise)


def random_adapter(rng, m, degenerate=0.3):
    return "".join(rng.choice(LETTERS + LETTERS.lower() + "X-") if rng.random() < degenerate else rng.choice("ACGT") for _ in range(m))


def host_cases(seed=20240, count=1500):
    """(read, adapter, scheme, wildcards) for the host program and the plain-int32 kernels: every letter, junk bytes, noisy reads,
    adapters of 1 to 130 rows, affine and linear schemes, both modes, empty strings."""
    rng = random.Random(seed)
    cases = [("", "ACGT", SCHEMES[0], True), ("ACGT", "", SCHEMES[0], True), ("NNNN", "NNNN", SCHEMES[0], True),
             ("NNNN", "NNNN", SCHEMES[0], False), ("ACGTACGT", "NNNN", SCHEMES[0], True), ("AC--GT", "ACNNGT", SCHEMES[0], True)]
    while len(cases) < count:
        m = rng.choice([1, 2, 5, 7, 8, 9, 17, 22, 28, 31, 60, 130])
        n = rng.choice([1, 3, 10, 40, 150, 300])
        kind = rng.randrange(4)
        ad = [UMI28, PRIMER22, SPACER31][rng.randrange(3)] if kind == 0 else random_adapter(rng, m, rng.choice([0.0, 0.1, 0.3, 0.8]))
        if rng.random() < 0.7 and n >= len(ad):
            rd = read_with(rng, n, ad, rng.choice(["start", "end", "middle"]), edits=rng.randrange(0, 5), noise=rng.choice([0.0, 0.05]))
        else:
            rd = random_bases(rng, n, rng.choice([0.0, 0.1]))
        cases.append((rd, ad, rng.choice(SCHEMES), rng.random() < 0.8))
    return cases
