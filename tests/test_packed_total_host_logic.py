"""ScanParams.packed_total: the host logic of the packed route when the prefilter takes EVERY adapter list over the plane
(pc_prefilter_packed_any) -- over the oracle-backed stand-in, no GPU.  With an adapter that holds an N the reads stay
packed, nothing is refused, and trims and middle hits equal the byte route's; without the switch the same list is refused
as before (tests/test_packed_pipeline_host_logic.py, unchanged)."""
import numpy as np
import torch

from porechop_amd.io import pack_reads
from porechop_amd.pipeline import AdapterSet, DeviceReads, Pipeline, ScanParams
from tests.cpu_aligner import OracleAligner
from tests.longgen import Y_BOTTOM, Y_TOP
from tests.test_packed_pipeline_host_logic import reads_for_test

BASES = {ord(c): i for c, i in zip("ACGTUacgtu", [0, 1, 2, 3, 3, 0, 1, 2, 3, 3])}


def min_edits_wildcard(text, adapter):
    """Fewest unit-cost edits between the adapter (global) and a substring of text (bytes 'A' 'C' 'G' 'T'), adapter letters
    that are not A/C/G/T/U matching everything: Myers' recurrence on Python integers -- the contract of
    prefilter_packed_kernel (porechop_amd/csrc/pc_prefilter.hip)."""
    m = len(adapter)
    full = (1 << m) - 1
    peq = [0, 0, 0, 0]
    for r, ch in enumerate(adapter):
        for code in range(4):
            if BASES.get(ch, code) == code:
                peq[code] |= 1 << r
    row = {ord("A"): peq[0], ord("C"): peq[1], ord("G"): peq[2], ord("T"): peq[3]}
    pv, mv, score, best, hi = full, 0, m, m, 1 << (m - 1)
    for ch in text:
        eq = row[ch]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & full)
        mh = pv & xh
        score += 1 if ph & hi else (-1 if mh & hi else 0)
        ph, mh = (ph << 1) & full, (mh << 1) & full
        pv = mh | (~(xv | ph) & full)
        mv = ph & xv
        best = min(best, score)
    return best


class TotalAligner(OracleAligner):
    """prefilter_rows(packed=True, total=True): the plane's bytes (non-bases of the reads as 'A') against the adapters with
    their non-base letters as wildcards; never None."""

    def prefilter_rows(self, arena, win_off, win_len, max_len, adapters, max_edits, stream=None, packed=False, total=False):
        if not (packed and total):
            return super().prefilter_rows(arena, win_off, win_len, max_len, adapters, max_edits, stream, packed=packed)
        nb = int((win_off + win_len.to(torch.int64)).max().item()) if win_off.numel() else 0
        text = self._plane_bytes(arena, nb).tobytes()
        wo, wl = win_off.numpy(), win_len.numpy()
        dense = torch.zeros((len(adapters), wo.shape[0]), dtype=torch.bool)
        for j, (ad, k) in enumerate(zip(adapters, max_edits)):
            seq = self.adapters[int(ad)]
            for w in range(wo.shape[0]):
                if wl[w] > 0 and len(seq) > 0:
                    dense[j, w] = k < 0 or min_edits_wildcard(text[wo[w]:wo[w] + wl[w]], seq) <= k
        rows = torch.nonzero(dense.any(dim=0)).flatten()
        return rows, dense[:, rows].t().contiguous()


def test_the_wildcard_recurrence_equals_the_oracle_where_there_is_no_wildcard(oracle):
    rng = np.random.default_rng(2)
    for m in (1, 4, 22, 28, 40):
        ad = "".join("ACGT"[i] for i in rng.integers(0, 4, m))
        texts = ["".join("ACGT"[i] for i in rng.integers(0, 4, n)) for n in (1, 5, 30, 200)]
        texts.append(texts[-1][:90] + ad[:m - m // 4] + texts[-1][90:])
        arr = np.frombuffer("".join(texts).encode() + b"N" * 16, dtype=np.uint8)
        lens = np.array([len(t) for t in texts], dtype=np.int32)
        offs = (np.cumsum(lens, dtype=np.int64) - lens).astype(np.int64)
        want = oracle.min_edits_many(arr, offs, lens, ad)
        assert [min_edits_wildcard(t.encode(), ad.encode()) for t in texts] == want.tolist()
    assert min_edits_wildcard(b"TTTTACGTAAGTTTTT", b"ACGTNNGT") == 0 and min_edits_wildcard(b"TTTTACGTAAGTTTTT", b"ACGTCCGT") == 2


def run(oracle, sets, packed, total):
    p = ScanParams(packed_total=total)
    pl = Pipeline(sets, p, aligner=TotalAligner(oracle, p.scores))
    reads = reads_for_test()
    blob = "".join(reads).encode()
    arena = np.frombuffer(blob + b"N" * 64, dtype=np.uint8).copy()
    lens = torch.tensor([len(r) for r in reads], dtype=torch.int32)
    off = torch.cumsum(lens.to(torch.int64), 0) - lens.to(torch.int64)
    if packed:
        pk, exc = pack_reads(arena, len(blob))
        dr = DeviceReads.packed_only(pl.aligner, torch.from_numpy(pk), len(blob), torch.from_numpy(exc), off, lens, end_size=pl.p.end_size)
        assert dr.arena is None
    else:
        dr = DeviceReads(torch.from_numpy(arena), off, lens)
    bs, be = pl.phase_a(dr)
    matching = pl.matching_sets(bs, be)
    st, et = pl.phase_b(dr, matching)[:2]
    h = pl.phase_c(dr, st, et, matching, prefilter=True)
    return (matching, st.tolist(), et.tolist(), sorted(zip(h.read.tolist(), h.adapter.tolist(), h.start.tolist(), h.end.tolist()))), dict(pl.stats), dr


def test_an_adapter_list_with_an_n_stays_on_the_packed_route_when_asked_to(oracle):
    with_n = Y_TOP[:10] + "N" + Y_TOP[11:]
    sets = [AdapterSet("SQK-NSK007", ("SQK-NSK007_Y_Top", Y_TOP), ("SQK-NSK007_Y_Bottom", Y_BOTTOM)),
            AdapterSet("with N", ("n_top", with_n), None)]
    want, _, _ = run(oracle, sets, packed=False, total=False)
    assert len(want[0]) == 2 and len(want[3]) >= 10                 # both sets match: the N adapter is in the middle scan's list
    got, stats, dr = run(oracle, sets, packed=True, total=True)
    assert got == want
    assert dr.arena is None and "packed_route_refused" not in stats
    assert 0 < stats["bases_unpacked_after_prefilter"] < 0.8 * dr.nbases
    # the default: the same list is refused and everything is unpacked
    got, stats, dr = run(oracle, sets, packed=True, total=False)
    assert got == want
    assert stats.get("packed_route_refused", 0) >= 1 and dr.arena is not None
