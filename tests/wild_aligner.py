"""TEST INFRASTRUCTURE: the stand-in aligner of tests/cpu_aligner.py with its alignments taken from tests/wild_ref.py instead of
the oracle, so that the host logic above the C ABI runs with IUPAC wildcards on a machine without a GPU.  Never imported by
the product."""
import numpy as np

from tests import wild_ref
from tests.cpu_aligner import OracleAligner


class WildAligner(OracleAligner):
    def __init__(self, scores=(3, -6, -5, -2), wildcards=False):
        OracleAligner.__init__(self, None, scores)
        self.wildcards = bool(wildcards)

    def set_wildcards(self, enabled=True):
        self.wildcards = bool(enabled)

    def _align(self, arena, woff, wlen, ad):
        return self._align_now(arena, woff, wlen, ad)

    def _align_now(self, arena, woff, wlen, ad):
        raw = arena.tobytes()
        pairs = [(raw[int(o):int(o) + int(n)], self.adapters[ad]) for o, n in zip(woff, wlen)]
        rec, _ = wild_ref.align_many(pairs, self.scores, wildcards=self.wildcards)
        return np.ascontiguousarray(rec, dtype=np.int32)

    def prefilter(self, *a, **k):
        raise NotImplementedError("the stand-in has no prefilter under the wildcard rule")
