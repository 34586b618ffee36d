"""TEST INFRASTRUCTURE: the stand-in aligner of tests/wild_aligner.py plus the two UMI methods of the Aligner interface
(umi_span, umis), answered by tests/umi_ref.py over tests/wild_ref.py's paths, so that Pipeline.end_umis and the runner's UMI
route run on a machine without a GPU.  Never imported by the product."""
import torch

from tests import umi_ref
from tests.wild_aligner import WildAligner


class UmiAligner(WildAligner):
    umi = True

    def umi_span(self, adapter_index):
        return umi_ref.span(self.adapters[int(adapter_index)], self.wildcards)

    def umis(self, arena, win_off, win_len, adapter_index, side, rule=None, max_len=None, stream=None):
        if not self.wildcards or self.umi_span(adapter_index) is None or side not in (0, 1):
            raise RuntimeError("pc_umi_extract failed: bad argument (-3)")
        raw = arena.cpu().numpy().tobytes()
        windows = [raw[int(o):int(o) + int(n)] for o, n in zip(win_off.tolist(), win_len.tolist())]
        recs, umi = umi_ref.umi_many(windows, self.adapters[int(adapter_index)], self.scores, side, rule)
        return torch.from_numpy(recs), torch.from_numpy(umi)
