"""The exhaustive prefilter over the 2-bit plane against the byte route it replaces (diagnostic, GPU).
One process, the headline's reads (8-kb reads, 90 % / 50 % end adapters, 1 % chimeras) and its four middle adapters at
--middle_threshold 85, where no piece has seeds:
  (a) pc_prefilter_device over the unpacked bytes, seed stage off (PC_PF_NO_SEEDS=1: prefilter_kernel over every piece),
  (b) the pc_unpack_device pass that made those bytes,
  (c) pc_prefilter_packed_any over the plane (prefilter_packed_kernel over every piece).
(a) and (c) are pc_get_timing's kind 4 ("prefilter"), (b) is bracketed by events; the calls alternate, medians are reported.
Criterion: (c) <= 1.05 x (a).
usage: prefilter_packed_total.py [reads] [repeats] [output file]"""
import os
import statistics
import sys

os.environ["PC_PF_NO_SEEDS"] = "1"           # read once per process by the library: before its first prefilter call
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from porechop_amd.io import pack_reads
from porechop_amd.panel import load_panel
from porechop_amd.pipeline import Pipeline, ScanParams
from porechop_amd.synth import make_reads

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                              "prefilter_packed_total.txt")
THRESHOLD, READ_LEN = 85.0, 8000
dev = torch.device("cuda")
pl = Pipeline(load_panel(), ScanParams(middle_threshold=THRESHOLD), device=dev)
al = pl.aligner
reads = make_reads(n, READ_LEN, seed=3, start_frac=0.9, end_frac=0.5, chimera_frac=0.01, device=dev)
bs, be = pl.phase_a(reads, torch.arange(min(n, 10000), device=dev))
matching = pl.matching_sets(bs, be)
ads = pl.middle_adapter_list(matching)
ids = [pl.seq_index[a[1]] for a in ads]
ks = [al.max_edits(len(a[1]), THRESHOLD) for a in ads]
nbases = n * READ_LEN
lines = ["reads %d x %d bases, --middle_threshold %.0f, middle adapters %s, max edits %s, PC_PF_NO_SEEDS=1, %s"
         % (n, READ_LEN, THRESHOLD, [len(a[1]) for a in ads], ks, torch.cuda.get_device_name(0))]
print(lines[0], flush=True)

# the plane, from the same bases (packed on the host a slice at a time, as an upload would)
plane = torch.zeros((nbases + 15) // 16 * 4 + 64, dtype=torch.uint8, device=dev)
nexc, step = 0, 1 << 28                      # (a multiple of 16 bases: slices start on a dword of the plane)
for s in range(0, nbases, step):
    e = min(nbases, s + step)
    pk, exc = pack_reads(reads.arena[s:e].cpu().numpy())
    plane[s // 4:s // 4 + pk.size] = torch.from_numpy(pk).to(dev)
    nexc += int(exc.size)
assert nexc == 0                             # synthetic reads hold A/C/G/T only: the two masks must be equal bit for bit
off, length = reads.off.contiguous(), reads.length.contiguous()
unpacked = torch.empty(nbases + 64, dtype=torch.uint8, device=dev)
al.set_timing(True)


def bytes_route():
    al.get_timing()
    m = al.prefilter_mask(unpacked, off, length, READ_LEN, ids, ks)
    return m, al.get_timing()["prefilter"][0]


def unpack_pass():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    al.unpack_device(plane, nbases, None, arena=unpacked)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def plane_route():
    al.get_timing()
    m = al.prefilter_mask_packed(plane, off, length, READ_LEN, ids, ks, total=True)
    return m, al.get_timing()["prefilter"][0]


unpack_pass()
assert torch.equal(unpacked[:nbases], reads.arena[:nbases])
m_a, _ = bytes_route()                       # warm-up of every shape, and the masks
m_c, _ = plane_route()
torch.cuda.synchronize()
assert torch.equal(m_a, m_c), "the two routes' masks differ"
survivors = int((m_c != 0).any(dim=1).sum())
ta, tb, tc = [], [], []
for _ in range(repeats):
    tb.append(unpack_pass())
    ta.append(bytes_route()[1])
    tc.append(plane_route()[1])
a, b, c = statistics.median(ta), statistics.median(tb), statistics.median(tc)
lines += ["masks equal bit for bit; %d of %d reads survive" % (survivors, n),
          "(a) pc_prefilter_device, exhaustive, bytes : median %.3f ms  (min %.3f, max %.3f, %d runs)" % (a, min(ta), max(ta), repeats),
          "(b) pc_unpack_device                       : median %.3f ms  (min %.3f, max %.3f)" % (b, min(tb), max(tb)),
          "(c) pc_prefilter_packed_any, plane         : median %.3f ms  (min %.3f, max %.3f)" % (c, min(tc), max(tc)),
          "(c) / (a) = %.4f   criterion (c) <= 1.05 x (a): %s" % (c / a, "met" if c <= 1.05 * a else "NOT met"),
          "pair-columns per second: (a) %.3e  (c) %.3e" % (n * len(ids) * READ_LEN / (a / 1e3), n * len(ids) * READ_LEN / (c / 1e3))]
print("\n".join(lines[1:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
pl.close()
