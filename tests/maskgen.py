"""TEST INFRASTRUCTURE: reads for the mask rounds of the middle scan (csrc/pc_mask_rule.h, Pipeline.phase_c).

Random reads with 0 to 3 junctions each.  A junction is a copy (now and then mutated) of one of the four headline adapters,
a chimera junction (22-mer then 28-mer), or one of two OVERLAID junctions: the 33-mer laid over the 28-mer's 22 shared bases
and the 30-mer laid over the 22-mer's 13, so that two adapters of different sets hit overlapping intervals and the mask of
the first hit touches the record of the second.  Some reads carry a hit at their very first and very last bases, some the
same adapter twice (two rounds for one adapter)."""
import random

Y_TOP = "AATGTACTTCGTTCAGTTACGTATTGCT"                # 28, SQK-NSK007 start
Y_BOTTOM = "GCAATACGTAACTGAACGAAGT"                   # 22, SQK-NSK007 end
P2_START = "CTTCGTTCAGTTACGTATTGCTGGCGTCTGCTT"        # 33, 1D^2 part 2 start: Y_TOP[6:] + 11 bases
P2_END = "CACCCAAGCAGACGCCAGCAATACGTAACT"             # 30, 1D^2 part 2 end: 17 bases + Y_BOTTOM[:13]
SETS = ("SQK-NSK007", "1D^2 part 2")
# ... and a third set, after them in the panel, whose sequences share exactly ONE base with the 28-mer's ends: a hit of the
# 28-mer then masks one column of the other record, the mask's last or its first (touching_reads)
SETS3 = SETS + ("Barcode 2 (reverse)",)
BC02_REV = "ACAGACGACTACAAACGGAATCGA"                 # ends with the 28-mer's first base
BC02 = "TCGATTCCGTTTGTAGTCGTCTGT"                     # starts with the 28-mer's last base
OVER_TOP = Y_TOP[:6] + P2_START                       # the 28-mer and the 33-mer, both whole, 22 bases shared
OVER_BOTTOM = P2_END + Y_BOTTOM[13:]                  # the 30-mer and the 22-mer, both whole, 13 bases shared
assert Y_TOP[6:] == P2_START[:22] and P2_END[17:] == Y_BOTTOM[:13]
assert BC02_REV[-1] == Y_TOP[0] and BC02[0] == Y_TOP[-1]


def _bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s, rate):
    out = []
    for ch in s:
        if rng.random() >= rate:
            out.append(ch)
            continue
        k = rng.randrange(3)
        if k == 0:
            out.append(rng.choice([c for c in "ACGT" if c != ch]))
        elif k == 2:
            out.append(ch + rng.choice("ACGT"))
    return "".join(out)


def junction(rng):
    kind = rng.randrange(8)
    if kind == 0:
        j = Y_BOTTOM + Y_TOP
    elif kind in (1, 2):
        j = OVER_TOP
    elif kind == 3:
        j = OVER_BOTTOM
    elif kind == 4:
        a = rng.choice((Y_TOP, Y_BOTTOM))
        j = a + _bases(rng, rng.randrange(0, 40)) + a         # the same adapter twice
    else:
        j = rng.choice((Y_TOP, Y_BOTTOM, P2_START, P2_END))
    return _mutate(rng, j, rng.choice((0.0, 0.0, 0.04, 0.08, 0.12)))


def reads(seed, n, lo=300, hi=1500):
    """n reads of lo..hi bases, about a third of them without a junction."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        length = rng.randrange(lo, hi + 1)
        k = rng.choice((0, 0, 1, 1, 2, 3))
        parts, left = [], length
        for _ in range(k):
            j = junction(rng)
            gap = _bases(rng, rng.randrange(0, max(1, left // (k + 1))))
            parts += [gap, j]
            left -= len(gap) + len(j)
        seq = "".join(parts) + _bases(rng, max(0, left))
        if i % 7 == 3:                                        # hits at the read's first and last bases
            seq = rng.choice((Y_TOP, OVER_TOP)) + seq + rng.choice((Y_BOTTOM, OVER_BOTTOM))
        elif i % 7 == 5:
            seq = P2_END + seq + Y_TOP
        out.append(seq)
    return out


def touching_reads(seed, n):
    """n reads in which a record of the third set of SETS3 meets the mask of the 28-mer's hit by exactly one column (even
    reads: the mask's last column, odd reads: its first) or by none (every fourth pair: the two copies side by side)."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        left, right = _bases(rng, rng.randrange(150, 400)), _bases(rng, rng.randrange(150, 400))
        share = 0 if i % 8 >= 6 else 1
        mid = (Y_TOP[:28 - share] + BC02) if i % 2 == 0 else (BC02_REV[:24 - share] + Y_TOP)
        out.append(left + mid + right)
    return out
