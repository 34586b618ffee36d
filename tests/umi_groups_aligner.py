"""TEST INFRASTRUCTURE: the stand-in aligner of tests/umi_aligner.py as the UMI-group tests need it -- WITHOUT umi_neighbours, so
that the runner's grouping takes the host route (umi_groups.neighbours_host) on a machine without a GPU -- and the end-to-end
case of those tests: ten hand-made reads for the kit of tests/umi_runner_case.py whose UMIs are chosen so that the groups can
be STATED BY HAND.  Never imported by the product."""
import random

from tests import umi_runner_case as case
from tests.umi_aligner import UmiAligner


class UmiGroupsAligner(UmiAligner):
    """UmiAligner as it is: it has no umi_neighbours."""


assert not hasattr(UmiGroupsAligner, "umi_neighbours")

S_A, E_A = "ACGACGACGACGACGA", "ACGTACGT"          # molecule A: three exact reads and one with a substituted base in the end UMI
E_A1 = "ACGTACGA"
S_B, E_B = "GGGGCCCCAAAAGCGC", "TTTTGGGG"          # molecule B: two reads, far from A
S_C = "CACACACAGAGAGAGA"                           # a read with the start UMI only: no key under "both"
S_N, E_N = "AAAACCCCGGGGACGA", "NACGTTGA"          # an N in the end UMI: a key that cannot be linked
E_D = "GATTACAG"                                   # a read with the end UMI only

# (start UMI bases or None, end UMI or None)
READS = [(S_A, E_A), (S_B, E_B), (S_A, E_A), (S_A, E_A1), (S_C, None), (S_A, E_A), (S_B, E_B), (S_N, E_N), (None, None), (None, E_D)]

K_A = case.start_umi(S_A) + "+" + E_A
K_A1 = case.start_umi(S_A) + "+" + E_A1
K_B = case.start_umi(S_B) + "+" + E_B
K_N = case.start_umi(S_N) + "+" + E_N

# by = "both" (the default for this panel), max_dist 2, directional.  Nodes by count, then key: K_A (3 reads), K_B (2), then the
# single-read keys K_A1 and K_N.  K_A founds group 1 and takes K_A1 (distance 1, 3 >= 2 * 1 - 1); K_B founds group 2; K_N has no
# edges and founds group 3.  Columns: name group key reads_of_key group_reads group_keys representative.
ROWS_BOTH = [("read_1", 1, K_A, 3, 4, 2, K_A), ("read_2", 2, K_B, 2, 2, 1, K_B), ("read_3", 1, K_A, 3, 4, 2, K_A),
             ("read_4", 1, K_A1, 1, 4, 2, K_A), ("read_6", 1, K_A, 3, 4, 2, K_A), ("read_7", 2, K_B, 2, 2, 1, K_B),
             ("read_8", 3, K_N, 1, 1, 1, K_N)]
GROUPS_BOTH = [(1, K_A), (2, K_B), (1, K_A), (1, K_A), None, (1, K_A), (2, K_B), (3, K_N), None, None]

# by = "start": the start UMIs alone.  S_A is held by four reads, S_B by two, S_C and S_N by one each; none within 2 edits of another.
U_A, U_B, U_C, U_N = (case.start_umi(u) for u in (S_A, S_B, S_C, S_N))
ROWS_START = [("read_1", 1, U_A, 4, 4, 1, U_A), ("read_2", 2, U_B, 2, 2, 1, U_B), ("read_3", 1, U_A, 4, 4, 1, U_A),
              ("read_4", 1, U_A, 4, 4, 1, U_A), ("read_5", 4, U_C, 1, 1, 1, U_C), ("read_6", 1, U_A, 4, 4, 1, U_A),
              ("read_7", 2, U_B, 2, 2, 1, U_B), ("read_8", 3, U_N, 1, 1, 1, U_N)]


def build():
    """-> records [(header, sequence)]"""
    rng = random.Random(1717)
    reads = []
    for k, (s, e) in enumerate(READS):
        body = "".join(rng.choice("ACGT") for _ in range(case.BODY))
        seq = (case.start_instance(s) if s is not None else "") + body + (case.end_instance(e) if e is not None else "")
        reads.append(("read_%d" % (k + 1), seq))
    return reads


def groups_text(rows):
    return "#name\tgroup\tkey\treads_of_key\tgroup_reads\tgroup_keys\trepresentative\n" + "".join("%s\t%d\t%s\t%d\t%d\t%d\t%s\n" % r for r in rows)
