"""TEST INFRASTRUCTURE: an oracle-backed stand-in with the Aligner interface (porechop_amd/batch.py),
so that the HOST logic above the C ABI (porechop_amd/pipeline.py, runner.py) can be checked on a
machine without a GPU.  Never imported by the product; the product's only aligner is the HIP library."""
import hashlib

import numpy as np
import torch

_MEMO = {}


class OracleAligner:
    def __init__(self, oracle, scores=(3, -6, -5, -2)):
        self.oracle = oracle
        self.scores = tuple(int(x) for x in scores)
        self.adapters = []

    def set_adapters(self, adapters):
        self.adapters = [a if isinstance(a, bytes) else a.encode() for a in adapters]
        self._arena = np.frombuffer(b"".join(self.adapters) + b"N", dtype=np.uint8)
        lens = np.array([len(a) for a in self.adapters], dtype=np.int32)
        self._len = lens
        self._off = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)

    def set_scores(self, scores):
        self.scores = tuple(int(x) for x in scores)

    def _align(self, arena, woff, wlen, ad):
        # many test cases re-run the same (windows, adapter, scores) job: remember the answers
        key = (self._digest(arena), hashlib.sha1(woff.tobytes()).digest(), hashlib.sha1(wlen.tobytes()).digest(),
               self.adapters[ad], self.scores)
        hit = _MEMO.get(key)
        if hit is None:
            hit = _MEMO[key] = self._align_now(arena, woff, wlen, ad)
        return hit

    @staticmethod
    def _digest(arena):
        return hashlib.sha1(arena.tobytes()).digest()      # every time: masked copies are edited in place

    def _align_now(self, arena, woff, wlen, ad):
        n = woff.shape[0]
        r9 = self.oracle.align_many(arena, woff, wlen, self._arena, np.full(n, self._off[ad]), np.full(n, self._len[ad], dtype=np.int32),
                                    self.scores)
        out = np.empty((n, 8), dtype=np.int32)
        out[:, :5] = r9[:, :5]
        out[:, 5] = r9[:, 5]
        out[:, 6] = r9[:, 6]
        out[:, 7] = r9[:, 8]
        return out

    def _records(self, arena, woff, wlen, ad, mode):
        rec = self._align(arena, woff, wlen, ad)
        if mode == 3:                       # MODE_SCORE: only the raw score is defined here (end cell omitted)
            out = np.zeros_like(rec)
            out[:, 0] = -2
            out[:, 4] = rec[:, 4]
            return out
        return rec

    def scan_device(self, arena, win_off, win_len, job_adapter, job_start, max_len, out, mode=0, stream=None, job_adapter_b=None):
        a = arena.cpu().numpy()
        wo, wl = win_off.cpu().numpy(), win_len.cpu().numpy()
        pos = 0
        for k, ad in enumerate(job_adapter):
            s, e = int(job_start[k]), int(job_start[k + 1])
            n = e - s
            out[pos:pos + n] = torch.from_numpy(self._records(a, wo[s:e], wl[s:e], int(ad), mode))
            pos += n
            if job_adapter_b is not None and int(job_adapter_b[k]) >= 0:
                out[pos:pos + n] = torch.from_numpy(self._records(a, wo[s:e], wl[s:e], int(job_adapter_b[k]), mode))
                pos += n

    def max_edits(self, adapter_len, threshold_percent):
        """Restatement of pc_prefilter_max_edits (include/porechop_amd.h) for machines without the library's GPU."""
        import math
        if adapter_len <= 0:
            return -1
        tau = (threshold_percent - 1e-6) / 100.0
        if not tau > 0.0:
            return adapter_len
        if tau >= 1.0:
            return 0
        return min(adapter_len, int(math.floor(adapter_len * (1.0 - tau) / tau + 1e-9)))

    def prefilter(self, arena, win_off, win_len, max_len, adapters, max_edits, stream=None):
        """The exact prefilter's contract, decided by the oracle's plain DP: True where the window holds the adapter
        within max_edits edits (max_edits < 0: every non-empty window)."""
        a = arena.cpu().numpy()
        wo, wl = win_off.cpu().numpy(), win_len.cpu().numpy()
        rows = []
        for ad, k in zip(adapters, max_edits):
            d = self.oracle.min_edits_many(a, wo, wl, self.adapters[int(ad)])
            ok = (d <= (k if k >= 0 else 1 << 30)) & (wl > 0) & (len(self.adapters[int(ad)]) > 0)
            rows.append(torch.from_numpy(ok))
        return torch.stack(rows) if rows else torch.zeros((0, wo.shape[0]), dtype=torch.bool)

    @staticmethod
    def _plane_bytes(plane, nbases):
        """The 2-bit plane as bytes, exceptions NOT applied (what the packed prefilter sees: non-bases read as 'A')."""
        pk = plane.cpu().numpy()[:(nbases + 3) // 4]
        codes = ((pk[:, None] >> (2 * np.arange(4, dtype=np.uint8))[None, :]) & 3).reshape(-1)[:nbases]
        return np.frombuffer(b"ACGT", dtype=np.uint8)[codes]

    def unpack_device(self, packed, nbases, exceptions, arena=None, pad=64, stream=None):
        raw = self._plane_bytes(packed, int(nbases)).copy()
        if exceptions is not None and exceptions.numel():
            raw[exceptions.cpu().numpy()] = ord("N")
        return torch.from_numpy(np.concatenate([raw, np.full(pad, ord("N"), dtype=np.uint8)]))

    def unpack_windows(self, plane, exceptions, src_off, length, dst, dst_off, pad=ord("N"), stream=None):
        so, ln, do = src_off.cpu().numpy(), length.cpu().numpy(), dst_off.cpu().numpy()
        nb = int((so + ln).max()) if so.size else 0
        raw = self._plane_bytes(plane, nb).copy()
        if exceptions is not None and exceptions.numel():
            e = exceptions.cpu().numpy()
            raw[e[e < nb]] = ord("N")
        out = dst.cpu().numpy().copy()
        for i in range(so.size):
            out[do[i]:do[i + 1]] = pad
            out[do[i]:do[i] + ln[i]] = raw[so[i]:so[i] + ln[i]]
        dst.copy_(torch.from_numpy(out))
        return dst

    def prefilter_rows(self, arena, win_off, win_len, max_len, adapters, max_edits, stream=None, packed=False):
        if packed:                                     # arena is the plane: the contract of pc_prefilter_packed
            if any(set(self.adapters[int(a)].upper()) - set(b"ACGTU") for a in adapters):
                return None
            nb = int((win_off + win_len.to(torch.int64)).max().item()) if win_off.numel() else 0
            arena = torch.from_numpy(np.concatenate([self._plane_bytes(arena, nb), np.full(64, ord("N"), dtype=np.uint8)]))
        dense = self.prefilter(arena, win_off, win_len, max_len, adapters, max_edits)
        rows = torch.nonzero(dense.any(dim=0)).flatten()
        return rows, dense[:, rows].t().contiguous()

    def sync(self, stream=None):
        pass

    def set_length_hint(self, typical_len):
        pass

    def set_timing(self, enabled=True):
        pass

    def close(self):
        pass
