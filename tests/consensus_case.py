"""TEST INFRASTRUCTURE: the end-to-end case of the UMI-consensus tests -- eleven hand-made reads for the kit of
tests/umi_runner_case.py whose bodies are copies of two originals with edits placed BY HAND, so that the consensus FASTA and
its report can be stated by hand.  The CPU test runs it on the stand-in aligner (no consensus_round: the host route), the GPU
test on the library; both must write these bytes.  Never imported by the product.

Every read loses its adapters and extra_end_trim = 2 bases on either side: a member's sequence is body[2:-2], 236 bases of 240.

Molecule A, five reads under one key (group 1: the key with the most reads), in input order
    A1  the original                       A2  the original
    A3  base 60 substituted                X   an UNRELATED body under A's UMIs       A4  base 100 substituted
  All are 236 bases, so the order by (length, input order) is the input order and the lower median of five is the third: A3 is
  the template of round 1.  X is about half its length away: rejected (30 %).  voters = A3 + A1, A2, A4 = 4.  Column 60 holds
  three votes for the original's base against the template's one, column 100 three (A1, A2, A3) against A4's one: round 1 calls
  the original.  It differs from A3, so round 2 runs with the original as the template and all five reads as members: X is
  rejected again, used = 4, and the call returns its template: rounds = 2.
Molecule D, three reads (group 2)
    D1  the original (236)    D2  base 150 deleted (235)    D3  a base inserted before base 90 (237)
  By (length, input order): D2, D1, D3 -- the lower median is D1.  voters = 3.  D2's deletion has one vote against two bases;
  D3's insertion fills slot 0 of its gap with one vote, and 2 * 1 > 3 is false: not emitted.  Round 1 returns its template:
  rounds = 1.
Molecule B, two reads (group 3): fewer than min_reads = 3.  The key with an N (group 4): one read."""
import random

from tests import umi_runner_case as case
from tests.umi_aligner import UmiAligner


class ConsensusAligner(UmiAligner):
    """UmiAligner as it is: it has neither umi_neighbours nor consensus_round."""


assert not hasattr(ConsensusAligner, "consensus_round")

S_A, E_A = "ACGACGACGACGACGA", "ACGTACGT"
S_D, E_D = "CACACACAGAGAGAGA", "GGTTGGTT"
S_B, E_B = "GGGGCCCCAAAAGCGC", "TTTTGGGG"
S_N, E_N = "AAAACCCCGGGGACGA", "NACGTTGA"
K_A, K_D, K_B, K_N = (case.start_umi(s) + "+" + e for s, e in ((S_A, E_A), (S_D, E_D), (S_B, E_B), (S_N, E_N)))

_rng = random.Random(1818)


def _body():
    return "".join(_rng.choice("ACGT") for _ in range(case.BODY))


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


ORIG_A, ORIG_D, UNRELATED, BODY_B1, BODY_B2, BODY_N = (_body() for _ in range(6))


def _sub(body, at):
    return body[:at] + _other(body[at]) + body[at + 1:]


# (start UMI, end UMI, body)
READS = [(S_A, E_A, ORIG_A), (S_D, E_D, ORIG_D), (S_A, E_A, ORIG_A), (S_B, E_B, BODY_B1), (S_A, E_A, _sub(ORIG_A, 60)),
         (S_D, E_D, ORIG_D[:150] + ORIG_D[151:]), (S_A, E_A, UNRELATED), (S_N, E_N, BODY_N), (S_A, E_A, _sub(ORIG_A, 100)),
         (S_D, E_D, ORIG_D[:90] + _other(ORIG_D[90]) + ORIG_D[90:]), (S_B, E_B, BODY_B2)]

SEQUENCES = [ORIG_A[2:-2].encode(), ORIG_D[2:-2].encode(), None, None]
FASTA = (">umi_group_1 key=%s reads=5 used=4 rounds=2 length=236\n%s\n" % (K_A, ORIG_A[2:-2]) +
         ">umi_group_2 key=%s reads=3 used=3 rounds=1 length=236\n%s\n" % (K_D, ORIG_D[2:-2]))
TSV = ("#group\trepresentative\tmembers\tused\trejected\tskipped\trounds\tlength\tstatus\n"
       "1\t%s\t5\t4\t1\t0\t2\t236\tcalled\n" % K_A +
       "2\t%s\t3\t3\t0\t0\t1\t236\tcalled\n" % K_D +
       "3\t%s\t2\t0\t0\t0\t0\t0\tfew_reads\n" % K_B +
       "4\t%s\t1\t0\t0\t0\t0\t0\tfew_reads\n" % K_N)


def build():
    """-> records [(header, sequence)]"""
    return [("read_%d" % (k + 1), case.start_instance(s) + body + case.end_instance(e)) for k, (s, e, body) in enumerate(READS)]
