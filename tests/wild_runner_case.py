"""TEST INFRASTRUCTURE: the end-to-end case of the IUPAC-wildcard tests -- a UMI adapter set at both ends of 40 short reads plus
one chimera with the start adapter in its middle -- with the trims and the split STATED BY HAND from where the instances were
planted (extra_end_trim 2; a start adapter in the middle takes 100 bases before it and 10 behind it)."""
import random

from tests import wildgen

START = wildgen.UMI28              # twelve V: 16 of 28 rows can match without wildcards -- 57 %, below every threshold
END = wildgen.PRIMER22
N_SHORT = 40
BODY = 240
CHIMERA_BODY = 1500


def adapter_sets():
    from porechop_amd.pipeline import AdapterSet
    return [AdapterSet("UMI kit", ("UMI_start", START), ("UMI_end", END))]


def _body(rng, n):
    # (plain random bases: an instance is aligned in full, so what follows it cannot move the alignment's end)
    return "".join(rng.choice("ACGT") for _ in range(n))


def build():
    """-> (reads, expected pieces with wildcards on): expected[r] is the list of sequences read r leaves in the output."""
    rng = random.Random(505)
    reads, expected = [], []
    for _ in range(N_SHORT):
        body = _body(rng, BODY)
        reads.append(wildgen.instance(rng, START) + body + wildgen.instance(rng, END))
        expected.append([body[2:-2]])                         # adapter + extra_end_trim at either end
    b1, b2 = _body(rng, CHIMERA_BODY), _body(rng, CHIMERA_BODY)
    reads.append(wildgen.instance(rng, START) + b1 + wildgen.instance(rng, START) + b2 + wildgen.instance(rng, END))
    # trimmed read = b1[2:] + instance + b2[:-2]; the hit is [len(b1) - 2, len(b1) + 26); a START adapter's bad side is the left
    expected.append([b1[2:len(b1) - 100], b2[10:-2]])
    return reads, expected


def write_fastq(path, reads):
    with open(path, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@read_%d\n%s\n+\n%s\n" % (i + 1, r, "5" * len(r)))
    return str(path)


def read_fastq(path):
    lines = open(path).read().split("\n")
    return list(zip((x[1:] for x in lines[0::4] if x), lines[1::4]))
