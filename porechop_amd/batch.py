"""Batch interface over the C ABI: many (window, adapter) pairs per call.

Host arrays are numpy; device-resident inputs are torch tensors (PyTorch is used only to own
HBM buffers and streams -- the compute is the HIP library).
"""
import ctypes

import numpy as np

from ._lib import check, load_library

RESULT_INTS = 8      # readStart, readEnd, adapterStart, adapterEnd, rawScore, matches, alignedLen, fullLen
MODE_AUTO, MODE_TRACE, MODE_TWO_PASS, MODE_SCORE, MODE_TRACE_AT = 0, 1, 2, 3, 4
SCAN_NO_SKIP_UNDERFILLED = 1  # scan_device(no_skip_underfilled=True): PC_SCAN_NO_SKIP_UNDERFILLED of include/porechop_amd.h
NO_FLOOR = -2 ** 31  # scan_device(floors=...): this job has no score floor (INT32_MIN)
DEFAULT_SCORES = (3, -6, -5, -2)   # porechop/porechop.py:145
INT_MIN = -2147483648


def format_result(rec):
    """One 8-int record -> the reference's 7-field string (formatted by the C side, i.e. by the
    same libc printf the reference uses through std::to_string)."""
    lib = load_library()
    arr = (ctypes.c_int32 * RESULT_INTS)(*[int(x) for x in rec])
    buf = ctypes.create_string_buffer(160)
    lib.pc_format_result(arr, buf, 160)
    return buf.value.decode()


def format_results(recs):
    """[n, 8] int32 records -> list of the reference's 7-field strings (pc_format_results: one call for all)."""
    recs = np.ascontiguousarray(recs, dtype=np.int32).reshape(-1, RESULT_INTS)
    n = int(recs.shape[0])
    if n == 0:
        return []
    lib = load_library()
    buf = ctypes.create_string_buffer(161 * n)
    used = ctypes.c_int64()
    check(lib.pc_format_results(recs.ctypes.data, n, buf, 161 * n, ctypes.byref(used)), "pc_format_results")
    out = buf.raw[:used.value].decode("ascii").split("\n")
    out.pop()
    return out


def records_to_fields(recs):
    """[n,8] int32 -> what porechop/nanopore_read.py:476-491 (align_adapter) derives per call:
    full_adapter_identity, aligned_identity (float64), read_start, read_end (= field1 + 1)."""
    recs = np.asarray(recs)
    failed = recs[:, 0] == -1
    with np.errstate(divide="ignore", invalid="ignore"):
        m = recs[:, 5].astype(np.float64)
        aligned = 100.0 * m / recs[:, 6].astype(np.float64)
        full = 100.0 * m / recs[:, 7].astype(np.float64)
    read_start = recs[:, 0].copy()
    read_end = recs[:, 1] + 1
    full[failed] = 0.0
    aligned[failed] = 0.0
    read_end[failed] = 0
    return full, aligned, read_start, read_end


OP_LETTERS = "=XID"  # pc_align_paths' two-bit operations: equal, unequal, read base over a gap, adapter base over a gap


def decode_paths(heads, ops):
    """heads int[n, 4] and ops [n, pitch] (32-bit words of either signedness) as align_paths returns them, on the host
    -> n FORWARD operation strings ("===X=I=="): the words hold the steps in traceback order, sixteen to a word, the
    first in the lowest bits."""
    heads = np.asarray(heads).reshape(-1, 4)
    ops = np.ascontiguousarray(np.asarray(ops)).astype(np.int64) & 0xFFFFFFFF
    ops = ops.reshape(heads.shape[0], -1) if heads.shape[0] else ops.reshape(0, 0)
    out = []
    for h, row in zip(heads, ops):
        L = int(h[0])
        if L < 0 or L > 16 * row.shape[0]:
            raise ValueError("a path of %d steps does not fit %d words" % (L, row.shape[0]))
        k = np.arange(L)
        codes = (row[k // 16] >> (2 * (k % 16))) & 3
        out.append("".join(OP_LETTERS[c] for c in codes[::-1]))
    return out


def cigar(opstring):
    """"===X=I==" -> "3=1X1=1I2=" (an empty path: "")."""
    out, i = [], 0
    while i < len(opstring):
        j = i
        while j < len(opstring) and opstring[j] == opstring[i]:
            j += 1
        if opstring[i] not in OP_LETTERS:
            raise ValueError("not a path operation: %r" % opstring[i])
        out.append("%d%s" % (j - i, opstring[i]))
        i = j
    return "".join(out)


def expand_cigar(text):
    """The inverse of cigar()."""
    out, run = [], ""
    for ch in text:
        if ch.isdigit():
            run += ch
        else:
            if ch not in OP_LETTERS or not run:
                raise ValueError("not a run-length path: %r" % text)
            out.append(ch * int(run))
            run = ""
    if run:
        raise ValueError("not a run-length path: %r" % text)
    return "".join(out)


def render_alignment(read, adapter, head, opstring):
    """Three lines over the path's columns: the read's bases, a '|' under every '=', the adapter's bases; '-' where a
    row has a gap.  head = (path_len, read_first, adapter_first, opens) as align_paths returns it."""
    read = read.decode() if isinstance(read, bytes) else read
    adapter = adapter.decode() if isinstance(adapter, bytes) else adapter
    j, i = int(head[1]), int(head[2])
    top, mid, bot = [], [], []
    for op in opstring:
        if op in "=X":
            top.append(read[j]); bot.append(adapter[i]); mid.append("|" if op == "=" else " ")
            j += 1; i += 1
        elif op == "I":
            top.append(read[j]); bot.append("-"); mid.append(" ")
            j += 1
        elif op == "D":
            top.append("-"); bot.append(adapter[i]); mid.append(" ")
            i += 1
        else:
            raise ValueError("not a path operation: %r" % op)
    return "\n".join(("".join(top), "".join(mid), "".join(bot)))


def letter_set(byte, wildcards):
    """The set of read codes (bit k: Dna5 code k = A, C, G, T/U, other) an adapter byte matches, with IUPAC wildcards on or
    off.  The table is the library's (csrc/pc_letters.h through pc_letter_set): there is no second copy of it here."""
    if isinstance(byte, (str, bytes)):
        byte = ord(byte)
    key = (int(byte), bool(wildcards))
    if key not in _LETTER_SETS:
        _LETTER_SETS[key] = int(load_library().pc_letter_set(key[0], 1 if key[1] else 0))
    return _LETTER_SETS[key]


_LETTER_SETS = {}                # (byte, mode) -> set, as the library answered


def mask_rule_gate(adapters, scores, wildcards):
    """May the mask rule (csrc/pc_mask_rule.h) be applied to a middle scan of these adapters under this scheme?  The
    library's answer (pc_mask_rule_gate; no device involved): every letter A/C/G/T/U, wildcards off, mismatch <= match."""
    seqs = [a if isinstance(a, bytes) else a.encode() for a in adapters]
    if any(b"\0" in a for a in seqs):
        return False
    arr = (ctypes.c_char_p * max(1, len(seqs)))(*seqs)
    match, mismatch, gap_open, gap_extend = (int(x) for x in scores)
    return bool(load_library().pc_mask_rule_gate(arr, len(seqs), match, mismatch, gap_open, gap_extend, 1 if wildcards else 0))


def mask_rule_must_realign(adapter, cur, read_start, read_end, mask_start, mask_end, floored_positive):
    """pcm::must_realign as the host compiles it (pc_mask_rule_must_realign): one record of one masked read."""
    return bool(load_library().pc_mask_rule_must_realign(int(adapter), int(cur), int(read_start), int(read_end), int(mask_start),
                                                         int(mask_end), 1 if floored_positive else 0))


class Aligner:
    """One GPU context: a scoring scheme + an adapter panel + scratch buffers."""
    fast_prefilter = True      # prefilter_rows is the device's exact prefilter (callers may put it in front of the middle scan)
    score_end_cell = True      # MODE_SCORE records carry the reference's end cell (row, column) besides the score
    reduce_takes_mask = True   # phase_b_reduce(traced_mask=...): pairs whose bit is clear are skipped without a load
    trace_at = True            # MODE_TRACE_AT: the traced record of a pair whose MODE_SCORE record (its end cell) is known
    end_rule = True            # scan_device(end_rule=..., job_side=...): end windows traced only where phase B's rule can trim
    paths = True               # align_paths / align_pairs_paths: records with the alignment's path (pc_align_paths)
    # (middle_paths, the method below, is its own flag: callers ask getattr(aligner, "middle_paths", False))

    def __init__(self, adapters, scores=DEFAULT_SCORES, device=-1, wildcards=False):
        self.lib = load_library()
        self._ctx = ctypes.c_void_p()
        check(self.lib.pc_create(ctypes.byref(self._ctx), device), "pc_create")
        self.scores = tuple(int(s) for s in scores)
        check(self.lib.pc_set_scores(self._ctx, *self.scores), "pc_set_scores")
        self.wildcards = False
        self.set_wildcards(wildcards)
        self.set_adapters(adapters)

    def set_adapters(self, adapters):
        """Replace the adapter table (indices used by later calls refer to the new list)."""
        self.adapters = [a if isinstance(a, bytes) else a.encode() for a in adapters]
        arr = (ctypes.c_char_p * max(1, len(self.adapters)))(*self.adapters)
        check(self.lib.pc_set_adapters(self._ctx, arr, len(self.adapters)), "pc_set_adapters")

    def set_scores(self, scores):
        """Replace the scoring scheme (match, mismatch, gap_open, gap_extend) of the live context (pc_set_scores): the
        adapter table and everything derived from it is worked out again at the next call."""
        scores = tuple(int(s) for s in scores)
        check(self.lib.pc_set_scores(self._ctx, *scores), "pc_set_scores")
        self.scores = scores

    def set_wildcards(self, enabled=True):
        """IUPAC wildcards in the adapters of the live context (pc_set_wildcards; off by default): an adapter letter stands for
        its set of bases, a read base that is not A/C/G/T/U matches nothing.  Everything derived from the panel is worked out
        again at the next call.  Every DP kernel takes the adapters as sets, the specialised score kernels included (compiled per
        pair as ever; declined only where the letter pairs outgrow the register plan)."""
        check(self.lib.pc_set_wildcards(self._ctx, 1 if enabled else 0), "pc_set_wildcards")
        self.wildcards = bool(enabled)

    def close(self):
        if self._ctx:
            self.lib.pc_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host buffers ------------------------------------------------------------------
    def align_host(self, arena, win_off, win_len, adapter_idx, mode=MODE_AUTO):
        """arena: bytes / uint8 array; win_off int64[n]; win_len int32[n]; adapter_idx int32[n]
        -> int32 [n, 8]"""
        arena = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) \
            else np.ascontiguousarray(arena, dtype=np.uint8)
        win_off = np.ascontiguousarray(win_off, dtype=np.int64)
        win_len = np.ascontiguousarray(win_len, dtype=np.int32)
        adapter_idx = np.ascontiguousarray(adapter_idx, dtype=np.int32)
        n = win_off.shape[0]
        out = np.zeros((n, RESULT_INTS), dtype=np.int32)
        check(self.lib.pc_align_batch_host(self._ctx, arena.ctypes.data, arena.size, win_off.ctypes.data,
                                           win_len.ctypes.data, adapter_idx.ctypes.data, n, mode,
                                           out.ctypes.data), "pc_align_batch_host")
        return out

    def align_pairs(self, pairs, mode=MODE_AUTO):
        """pairs: iterable of (read_str, adapter_index) -> int32 [n, 8]"""
        offs, lens, idx, chunks, pos = [], [], [], [], 0
        for rd, ai in pairs:
            b = rd if isinstance(rd, bytes) else rd.encode()
            offs.append(pos)
            lens.append(len(b))
            idx.append(ai)
            chunks.append(b)
            pos += len(b)
        return self.align_host(b"".join(chunks), offs, lens, idx, mode)

    # ---- device buffers (torch tensors on the GPU) --------------------------------------
    def scan_device(self, arena, win_off, win_len, job_adapter, job_start, max_len, out,
                    mode=MODE_AUTO, stream=None, job_adapter_b=None, floors=None, floors_b=None, end_rule=None, job_side=None,
                    no_skip_underfilled=False):
        """arena uint8[*], win_off int64[n], win_len int32[n]: CUDA(HIP) tensors describing n windows.
        job_adapter int32[k], job_start int64[k+1] (window ranges), optional job_adapter_b int32[k]
        (-1 = none): host numpy.  out int32[total,8] with total = sum n_k * (1 or 2), job order,
        adapter A's records before adapter B's.  Asynchronous; call sync().
        floors / floors_b int32[k] (MODE_TWO_PASS only; NO_FLOOR = none): a pair whose best score is below its job's floor is
        not traced and gets the record (-1, 0, ..., 0) (pc_scan_device_floored); every other record is unchanged.
        end_rule = (end_size, min_trim_size, extra_end_trim, end_threshold) with job_side int32[k] (0 = start windows, 1 = end
        windows; MODE_AUTO or MODE_TWO_PASS): a pair that cannot trim its read by phase B's rule is not traced and gets that
        same record (pc_scan_device_end_rule); every other record is unchanged.
        no_skip_underfilled (this call only): launches the library cuts into column chunks, because they do not fill the
        device, skip no adapter rows (pc_scan_device_floored_flags; the records are the same either way).  Only a call with
        floors skips rows at all, so with an end rule the option is an error and without floors it changes nothing."""
        import torch
        assert arena.is_cuda and win_off.is_cuda and win_len.is_cuda and out.is_cuda
        assert win_off.dtype == torch.int64 and win_len.dtype == torch.int32 and out.dtype == torch.int32
        job_adapter = np.ascontiguousarray(job_adapter, dtype=np.int32)
        job_start = np.ascontiguousarray(job_start, dtype=np.int64)
        jb = None
        if job_adapter_b is not None:
            jb = np.ascontiguousarray(job_adapter_b, dtype=np.int32)
        n = win_off.shape[0]
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if end_rule is not None:
            assert floors is None and floors_b is None and job_side is not None and not no_skip_underfilled
            from ._lib import EndRule
            rule = EndRule(int(end_rule[0]), int(end_rule[1]), int(end_rule[2]), float(end_rule[3]))
            side = np.ascontiguousarray(job_side, dtype=np.int32)
            assert side.shape[0] == len(job_adapter)
            check(self.lib.pc_scan_device_end_rule(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n,
                                                   job_adapter.ctypes.data, jb.ctypes.data if jb is not None else None,
                                                   job_start.ctypes.data, len(job_adapter),
                                                   int(max_len), mode, out.data_ptr(), ctypes.c_void_p(s),
                                                   ctypes.byref(rule), side.ctypes.data),
                  "pc_scan_device_end_rule")
            return
        if floors is not None or floors_b is not None:
            fa = np.ascontiguousarray(floors if floors is not None else np.full(len(job_adapter), NO_FLOOR), dtype=np.int32)
            fb = None if jb is None else np.ascontiguousarray(floors_b if floors_b is not None else np.full(len(job_adapter), NO_FLOOR),
                                                              dtype=np.int32)
            assert fa.shape[0] == len(job_adapter) and (fb is None or fb.shape[0] == len(job_adapter))
            args = (self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n,
                    job_adapter.ctypes.data, jb.ctypes.data if jb is not None else None, job_start.ctypes.data, len(job_adapter),
                    int(max_len), mode, out.data_ptr(), ctypes.c_void_p(s), fa.ctypes.data, fb.ctypes.data if fb is not None else None)
            if no_skip_underfilled:
                check(self.lib.pc_scan_device_floored_flags(*(args + (SCAN_NO_SKIP_UNDERFILLED,))), "pc_scan_device_floored_flags")
            else:
                check(self.lib.pc_scan_device_floored(*args), "pc_scan_device_floored")
            return
        check(self.lib.pc_scan_device(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n,
                                      job_adapter.ctypes.data, jb.ctypes.data if jb is not None else None,
                                      job_start.ctypes.data, len(job_adapter),
                                      int(max_len), mode, out.data_ptr(), ctypes.c_void_p(s)),
              "pc_scan_device")

    # ---- alignment paths (pc_paths.hip) ---------------------------------------------------------------------------------
    def longest_adapter(self):
        return max([len(a) for a in self.adapters] or [0])

    @staticmethod
    def _path_outputs(dev, n, pitch, stream):
        # -> zeroed (records, heads, ops) for n alignments on dev, and the stream handle the call runs on
        import torch
        records = torch.zeros((n, RESULT_INTS), dtype=torch.int32, device=dev)
        heads = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        ops = torch.zeros((n, max(1, pitch)), dtype=torch.int32, device=dev)
        return records, heads, ops, stream if stream is not None else torch.cuda.current_stream().cuda_stream

    def align_paths(self, arena, win_off, win_len, adapter_idx, max_len=None, stream=None):
        """The alignments of n (window, adapter) pairs WITH their paths (pc_align_paths).  arena uint8[*], win_off int64[n],
        win_len int32[n], adapter_idx int32[n]: CUDA tensors; max_len bounds win_len (None: its maximum, one host round
        trip).  -> (records int32[n, 8], heads int32[n, 4], ops int32[n, pitch]) CUDA tensors: the records are the scans',
        head = (path_len, read_first, adapter_first, opens), ops holds two bits per step in TRACEBACK order (the words'
        bits are the library's uint32; decode_paths turns them into forward strings).  Asynchronous; call sync()."""
        import torch
        assert arena.is_cuda and win_off.is_cuda and win_len.is_cuda and adapter_idx.is_cuda
        assert arena.dtype == torch.uint8 and win_off.dtype == torch.int64 and win_len.dtype == torch.int32 and adapter_idx.dtype == torch.int32
        assert win_off.is_contiguous() and win_len.is_contiguous() and adapter_idx.is_contiguous()
        n = int(win_off.shape[0])
        assert int(win_len.shape[0]) == n and int(adapter_idx.shape[0]) == n
        if max_len is None:
            max_len = int(win_len.max().item()) if n else 0
        max_len = int(max_len)
        pitch = max(1, (max_len + self.longest_adapter() + 15) // 16)
        records, heads, ops, s = self._path_outputs(arena.device, n, pitch, stream)
        check(self.lib.pc_align_paths(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), adapter_idx.data_ptr(), n,
                                      max_len, records.data_ptr(), heads.data_ptr(), ops.data_ptr(), pitch, ctypes.c_void_p(s)),
              "pc_align_paths")
        return records, heads, ops

    def align_pairs_paths(self, pairs):
        """pairs: iterable of (read_str, adapter_index) -> (records int32[n, 8], heads int32[n, 4], forward op strings):
        the host-side convenience beside align_pairs."""
        import torch
        offs, lens, idx, chunks, pos = [], [], [], [], 0
        for rd, ai in pairs:
            b = rd if isinstance(rd, bytes) else rd.encode()
            if not 0 <= int(ai) < len(self.adapters):
                raise ValueError("adapter index %r outside the table of %d" % (ai, len(self.adapters)))
            offs.append(pos)
            lens.append(len(b))
            idx.append(int(ai))
            chunks.append(b)
            pos += len(b)
        dev = torch.device("cuda")
        arena = torch.from_numpy(np.frombuffer(b"".join(chunks) + b"N", dtype=np.uint8).copy()).to(dev)
        recs, heads, ops = self.align_paths(arena, torch.tensor(offs, dtype=torch.int64, device=dev),
                                            torch.tensor(lens, dtype=torch.int32, device=dev),
                                            torch.tensor(idx, dtype=torch.int32, device=dev), max_len=max(lens or [0]))
        self.sync()
        heads = heads.cpu().numpy()
        return recs.cpu().numpy(), heads, decode_paths(heads, ops.cpu().numpy())

    # ---- UMI extraction (pc_paths.hip umi_kernel, pc_umi.h) --------------------------------------------------------------
    umi = True                 # umi_span / umis: the read bases under an adapter's degenerate letters (pc_umi_extract)

    def umi_span(self, adapter_index):
        """(first, last) -- the 0-based, inclusive rows of the adapter's UMI span under the context's letter rule: its first
        and last row whose letter set holds two or more bases -- or None (wildcards off included).  Host (pc_umi_span)."""
        first, last = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = self.lib.pc_umi_span(self._ctx, int(adapter_index), ctypes.byref(first), ctypes.byref(last))
        if rc < 0:
            check(rc, "pc_umi_span")
        return (int(first.value), int(last.value)) if rc == 1 else None

    def umis(self, arena, win_off, win_len, adapter_index, side, rule=None, max_len=None, stream=None):
        """The UMI of n end windows under ONE adapter (pc_umi_extract).  arena uint8[*], win_off int64[n], win_len int32[n]:
        CUDA tensors; side 0 = start windows, 1 = end windows; rule = (end_size, min_trim_size, extra_end_trim,
        end_threshold) or None (every alignment qualifies); max_len bounds win_len (None: its maximum, one host round
        trip).  -> (records int32[n, 8], umi int32[n, 4]) CUDA tensors: the scans' records and {status, first, len,
        covered} in window columns; status 0 complete, 1 no alignment, 2 does not qualify, 3 span clipped by the window.
        Asynchronous; call sync()."""
        import torch
        assert arena.is_cuda and win_off.is_cuda and win_len.is_cuda
        assert arena.dtype == torch.uint8 and win_off.dtype == torch.int64 and win_len.dtype == torch.int32
        assert win_off.is_contiguous() and win_len.is_contiguous()
        n = int(win_off.shape[0])
        assert int(win_len.shape[0]) == n
        if max_len is None:
            max_len = int(win_len.max().item()) if n else 0
        records = torch.zeros((n, RESULT_INTS), dtype=torch.int32, device=arena.device)
        umi = torch.zeros((n, 4), dtype=torch.int32, device=arena.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        r = None
        if rule is not None:
            from ._lib import EndRule
            r = ctypes.byref(EndRule(int(rule[0]), int(rule[1]), int(rule[2]), float(rule[3])))
        check(self.lib.pc_umi_extract(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n, int(max_len),
                                      int(adapter_index), int(side), r, records.data_ptr(), umi.data_ptr(), ctypes.c_void_p(s)),
              "pc_umi_extract")
        return records, umi

    # ---- UMI neighbours (pc_umi_groups.hip umi_neighbours_kernel, pc_umi_dist.h) -----------------------------------------
    def umi_neighbours(self, planes, lens, max_dist, cap=None, stream=None, strands=False):
        """Every pair i < j of n UMI keys whose edit distance is <= max_dist (pc_umi_neighbours).  planes int64[n, 2] (the bit
        planes p0, p1 of umi_groups.pack), lens int32[n]: CUDA tensors.  -> int32[m, 3] CUDA tensor {i, j, distance} of ALL
        such pairs, sorted by (i, j).  The list handed on is never incomplete: `found` is read after a sync, and when it is
        above cap (default: max(4 n, 1024)) the call is made again with cap = found -- a truncated list taken as proof of "no
        neighbour" would be wrong grouping.  max_len comes from lens.max().  A length outside 0..64 raises at the sync.
        strands=True (pc_umi_neighbours_stranded): -> int32[m, 4] {i, j, d, flip}, d the smaller of the distance as the keys stand
        and the distance with key j mirrored (umi_groups.mirror_key: the molecule's other strand), flip 1 iff the mirrored one
        is the smaller; the same retry."""
        import torch
        assert planes.is_cuda and lens.is_cuda and planes.dtype == torch.int64 and lens.dtype == torch.int32
        assert planes.is_contiguous() and lens.is_contiguous()
        n = int(lens.shape[0])
        assert tuple(planes.shape) == (n, 2)
        max_len = min(64, max(0, int(lens.max().item()))) if n else 0
        cap = max(4 * n, 1024) if cap is None else int(cap)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        found = torch.zeros(1, dtype=torch.int64, device=lens.device)
        entry, name, width = ((self.lib.pc_umi_neighbours_stranded, "pc_umi_neighbours_stranded", 4) if strands else
                              (self.lib.pc_umi_neighbours, "pc_umi_neighbours", 3))
        while True:
            pairs = torch.empty((cap, width), dtype=torch.int32, device=lens.device)
            check(entry(self._ctx, planes.data_ptr(), lens.data_ptr(), n, max_len, int(max_dist), pairs.data_ptr(), cap, found.data_ptr(),
                        ctypes.c_void_p(s)), name)
            self.sync(s)
            m = int(found.item())
            if m <= cap:
                break
            cap = m
        pairs = pairs[:m]
        if m:
            order = torch.argsort(pairs[:, 0].to(torch.int64) * n + pairs[:, 1].to(torch.int64))
            pairs = pairs[order]
        return pairs.contiguous()

    # ---- UMI consensus, one round (pc_consensus.hip, pc_consensus.h) ------------------------------------------------------
    def consensus_round(self, arena, tmpl_off, tmpl_len, member_off, member_len, member_group, band, max_err_pct, max_len=65535,
                        tmpl_counts=1, tmpl_arena=None, return_votes=False, stream=None, member_strand=None, qual_table=None):
        """One round of the UMI consensus (pc_consensus_round): every member aligned to its group's template inside `band`, the
        votes, the call.  arena: CUDA uint8 tensor holding the members (and the templates, unless tmpl_arena is given: another
        CUDA uint8 tensor).  tmpl_off int64[G], tmpl_len int32[G], member_off int64[M], member_len int32[M], member_group
        int32[M]: numpy arrays, the members ordered by group.  tmpl_counts: 1 when the template is a read of its group and
        stands for it among the voters, 0 when it is an earlier consensus.  member_strand: None, or uint8[M] (numpy) -- a member
        whose strand is 1 is read as its reverse complement (pc_consensus_round_stranded); None is pc_consensus_round itself.
        qual_table: None, or uint8[256] (numpy; each 0 .. 93, consensus.quality_table()) -- the call is pc_consensus_round_quality,
        and Round.qual holds one Phred value per byte of cons, gathered on the device with the index that gathers the sequences;
        a table entry above 93 raises before anything is launched.  None: the calls above, and Round.qual is None.
        -> consensus.Round (numpy): cons the consensus bytes of all groups back to back, lens[G], status[M] (0 accepted, 1
        rejected, 2 invalid), distance[M], voters[G], and votes (a list of uint32 arrays, 21 la + 16 counters per group) when
        return_votes, else None.  Only the sequences, lengths and per-member words come back from the device.  The call syncs:
        a length above max_len raises here.  A group that alone exceeds PC_CONSENSUS_SCRATCH_MB raises consensus.OverBudget
        with its index; bad arguments raise before anything is launched."""
        import torch
        from . import consensus as pcc
        assert arena.is_cuda and arena.dtype == torch.uint8 and arena.is_contiguous()
        tmpl_arena = arena if tmpl_arena is None else tmpl_arena
        assert tmpl_arena.is_cuda and tmpl_arena.dtype == torch.uint8 and tmpl_arena.is_contiguous()
        tmpl_off = np.ascontiguousarray(tmpl_off, dtype=np.int64)
        tmpl_len = np.ascontiguousarray(tmpl_len, dtype=np.int32)
        member_off = np.ascontiguousarray(member_off, dtype=np.int64)
        member_len = np.ascontiguousarray(member_len, dtype=np.int32)
        member_group = np.ascontiguousarray(member_group, dtype=np.int32)
        G, M = int(tmpl_len.shape[0]), int(member_len.shape[0])
        assert tmpl_off.shape == (G,) and member_off.shape == (M,) and member_group.shape == (M,)
        assert M == 0 or (np.all(np.diff(member_group) >= 0) and 0 <= int(member_group[0]) and int(member_group[-1]) < G), "members go in ordered by group"
        first = np.ascontiguousarray(np.searchsorted(member_group, np.arange(G + 1)), dtype=np.int64)
        la = np.clip(tmpl_len.astype(np.int64), 0, max(int(max_len), 0))
        cons_off = np.concatenate([[0], np.cumsum(pcc.cons_capacity(la))]).astype(np.int64)
        vote_off = np.concatenate([[0], np.cumsum(pcc.votes_per_group(la))]).astype(np.int64)
        dev = arena.device
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        cons = torch.empty(int(cons_off[-1]) + 16, dtype=torch.uint8, device=dev)
        lens = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
        voters = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
        out = torch.zeros((max(M, 1), 2), dtype=torch.int32, device=dev)
        votes = torch.zeros(int(vote_off[-1]) + 16, dtype=torch.int32, device=dev) if return_votes else None
        d_off, d_len, d_grp = (torch.from_numpy(x).to(dev) if M else torch.zeros(1, dtype=torch.from_numpy(x).dtype, device=dev)
                               for x in (member_off, member_len, member_group))
        qual = None
        if qual_table is not None:
            qual_table = np.ascontiguousarray(qual_table, dtype=np.uint8)
            assert qual_table.shape == (pcc.QUAL_ENTRIES,), "a quality table is uint8[256]"
            qual = torch.empty_like(cons)
        refused = ctypes.c_int64(-1)
        head = (self._ctx, arena.data_ptr(), tmpl_arena.data_ptr(), tmpl_off.ctypes.data, tmpl_len.ctypes.data, first.ctypes.data, G,
                d_off.data_ptr(), d_len.data_ptr(), d_grp.data_ptr())
        tail = (M, int(band), int(max_err_pct), int(max_len), int(tmpl_counts), cons.data_ptr(), lens.data_ptr(), voters.data_ptr(),
                out.data_ptr(), votes.data_ptr() if votes is not None else None, ctypes.byref(refused), ctypes.c_void_p(s))
        d_strand = None
        if member_strand is not None:
            member_strand = np.ascontiguousarray(member_strand, dtype=np.uint8)
            assert member_strand.shape == (M,)
            d_strand = torch.from_numpy(member_strand).to(dev) if M else torch.zeros(1, dtype=torch.uint8, device=dev)
        if qual is not None:
            rc = self.lib.pc_consensus_round_quality(*head, d_strand.data_ptr() if d_strand is not None else None, *tail,
                                                     qual_table.ctypes.data, qual.data_ptr())
        elif d_strand is None:
            rc = self.lib.pc_consensus_round(*head, *tail)
        else:
            rc = self.lib.pc_consensus_round_stranded(*head, d_strand.data_ptr(), *tail)
        if rc == -6:
            raise pcc.OverBudget(int(refused.value))
        check(rc, "pc_consensus_round")
        self.sync(s)
        h_lens = lens[:G].cpu().numpy()
        total = int(h_lens.sum())
        if total:
            d_lens = lens[:G].to(torch.int64)
            starts = torch.from_numpy(cons_off[:G]).to(dev) - (torch.cumsum(d_lens, 0) - d_lens)
            at = torch.repeat_interleave(starts, d_lens) + torch.arange(total, dtype=torch.int64, device=dev)
            h_cons = cons[at].cpu().numpy()
            h_qual = qual[at].cpu().numpy() if qual is not None else None
        else:
            h_cons = np.zeros(0, dtype=np.uint8)
            h_qual = np.zeros(0, dtype=np.uint8) if qual is not None else None
        h_out = out[:M].cpu().numpy()
        h_votes = None
        if votes is not None:
            flat = votes.cpu().numpy().view(np.uint32)
            h_votes = [flat[vote_off[g]:vote_off[g + 1]].copy() for g in range(G)]
        return pcc.Round(h_cons, h_lens, h_out[:, 0].copy(), h_out[:, 1].copy(), voters[:G].cpu().numpy(), h_votes, h_qual)

    # ---- paths of middle hits (pc_paths.hip) ----------------------------------------------------------------------------
    def middle_paths_cols(self, max_len):
        """The widest window (columns) a hit of middle_paths can have over reads of up to max_len bases
        (pc_middle_paths_cols: host arithmetic over the table and the scheme)."""
        cols = self.lib.pc_middle_paths_cols(self._ctx, int(max_len))
        if cols < 0:
            check(cols, "pc_middle_paths_cols")
        return int(cols)

    def middle_paths(self, arena, read_off, read_len, adapter_idx, read_end, mask_base, mask_count, intervals, max_len=None,
                     stream=None, ops_pitch=None):
        """The paths of n MIDDLE hits (pc_middle_paths), each from a bounded window of its masked trimmed read.  CUDA
        tensors: arena uint8[*]; per hit read_off int64[n], read_len int32[n] (the trimmed read), adapter_idx int32[n],
        read_end int32[n] (exclusive, trimmed-read coordinates), mask_base int64[n] and mask_count int32[n] into intervals
        int32[n, 2] (the hits' [start, end), sorted stably by read: the bases of rows mask_base .. + mask_count read as
        '-').  max_len bounds read_len (None: its maximum, one host round trip).  -> (records int32[n, 8], heads
        int32[n, 4], ops int32[n, pitch]) as align_paths, in trimmed-read coordinates.  Asynchronous; call sync()."""
        import torch
        tensors = (arena, read_off, read_len, adapter_idx, read_end, mask_base, mask_count, intervals)
        assert all(t.is_cuda and t.is_contiguous() for t in tensors)
        assert arena.dtype == torch.uint8 and read_off.dtype == torch.int64 and mask_base.dtype == torch.int64
        assert all(t.dtype == torch.int32 for t in (read_len, adapter_idx, read_end, mask_count, intervals))
        n = int(read_off.shape[0])
        assert all(int(t.shape[0]) == n for t in tensors[2:]) and tuple(intervals.shape) == (n, 2)
        if max_len is None:
            max_len = int(read_len.max().item()) if n else 0
        max_len = int(max_len)
        pitch = max(1, (self.middle_paths_cols(max_len) + self.longest_adapter() + 15) // 16) if ops_pitch is None else int(ops_pitch)
        records, heads, ops, s = self._path_outputs(arena.device, n, pitch, stream)
        check(self.lib.pc_middle_paths(self._ctx, arena.data_ptr(), read_off.data_ptr(), read_len.data_ptr(), adapter_idx.data_ptr(),
                                       read_end.data_ptr(), mask_base.data_ptr(), mask_count.data_ptr(), intervals.data_ptr(), n,
                                       max_len, records.data_ptr(), heads.data_ptr(), ops.data_ptr(), pitch, ctypes.c_void_p(s)),
              "pc_middle_paths")
        return records, heads, ops

    def floor_skipped(self, stream=None):
        """-> (pairs the last floored scan left untraced, those of all floored scans of this context) (pc_floor_skipped;
        waits for the stream)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        last, total = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self.lib.pc_floor_skipped(self._ctx, ctypes.c_void_p(s), ctypes.byref(last), ctypes.byref(total)), "pc_floor_skipped")
        return int(last.value), int(total.value)

    def set_row_skip_debug(self, enabled=True):
        """Count, per launch of a floored scan's score pass, the column pairs of the fast path and those with the rows below
        r0 computed (pc_set_row_skip_debug; read with row_skip_blocks)."""
        check(self.lib.pc_set_row_skip_debug(self._ctx, 1 if enabled else 0), "pc_set_row_skip_debug")

    def row_skip_blocks(self, stream=None):
        """-> (column pairs the fast path of the row-skipping launches ran since the last call, those with the lower rows on)
        (pc_row_skip_blocks; waits for the stream and clears the counters)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        n, on = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self.lib.pc_row_skip_blocks(self._ctx, ctypes.c_void_p(s), ctypes.byref(n), ctypes.byref(on)), "pc_row_skip_blocks")
        return int(n.value), int(on.value)

    def set_length_hint(self, typical_len):
        """Typical window length of the following whole-read scans (0 = about uniform): load balancing of the
        score pass only, never results (pc_set_length_hint)."""
        check(self.lib.pc_set_length_hint(self._ctx, int(max(0, typical_len))), "pc_set_length_hint")

    def set_int16_only(self, enabled=True):
        """Use the packed-int16 kernel variants even where the packed-fp16 ones are proven exact (cross-checks)."""
        check(self.lib.pc_set_int16_only(self._ctx, 1 if enabled else 0), "pc_set_int16_only")

    def set_timing(self, enabled=True):
        check(self.lib.pc_set_timing(self._ctx, 1 if enabled else 0), "pc_set_timing")

    def get_timing(self, stream=None):
        """-> dict kind -> (ms, launches, pairs) since the last call, for the kinds 'score' (generic
        score-only scan), 'plan', 'trace', 'score_spec' (run-time specialised score-only scan) and 'prefilter'
        (exact prefilter, all launches of a call as one region; its "pairs" are (window, adapter) pairs) and 'seed_scan' (the
        prefilter's seed scan alone: a sub-interval of 'prefilter'; its "pairs" are windows) and 'select' (the selection
        kernels of phase B's exact pruning)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        ms = (ctypes.c_double * 7)()
        ln = (ctypes.c_int64 * 7)()
        pr = (ctypes.c_int64 * 7)()
        check(self.lib.pc_get_timing(self._ctx, ctypes.c_void_p(s), ms, ln, pr), "pc_get_timing")
        return {k: (ms[i], ln[i], pr[i]) for i, k in enumerate(("score", "plan", "trace", "score_spec", "prefilter", "seed_scan", "select"))}

    def phase_b_reduce(self, records, n, job_record_offset, job_side, end_size, min_trim_size, extra_end_trim,
                       end_threshold, start_trim, end_trim, bins=None, barcode_threshold=0.0, barcode_diff=0.0,
                       require_two=False, call=None, stream=None, traced_mask=None):
        """Per-read reduction of end-window records on the device (pc_phase_b_reduce): records int32[*,8]
        written by scan_device for len(job_side) jobs over the same n reads; start_trim / end_trim (and call,
        when bins = [(start job or -1, end job or -1), ...] is given) are int32[n] CUDA tensors."""
        import torch
        assert records.is_cuda and start_trim.is_cuda and end_trim.is_cuda
        assert records.dtype == torch.int32 and start_trim.dtype == torch.int32 and end_trim.dtype == torch.int32
        off = np.ascontiguousarray(job_record_offset, dtype=np.int64)
        side = np.ascontiguousarray(job_side, dtype=np.int32)
        nb = 0 if bins is None else len(bins)
        bs = np.ascontiguousarray([b[0] for b in bins] if nb else [0], dtype=np.int32)
        be = np.ascontiguousarray([b[1] for b in bins] if nb else [0], dtype=np.int32)
        if nb:
            assert call is not None and call.is_cuda and call.dtype == torch.int32
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if traced_mask is not None:
            # traced_mask int64 [njobs, (n + 63) // 64]: the union of the selection rounds' masks (pc_phase_b_reduce_masked)
            assert traced_mask.is_cuda and traced_mask.dtype == torch.int64 and traced_mask.is_contiguous()
            assert tuple(traced_mask.shape) == (len(side), (int(n) + 63) // 64)
        check(self.lib.pc_phase_b_reduce_masked(self._ctx, records.data_ptr(), int(n), len(side), off.ctypes.data, side.ctypes.data,
                                                int(end_size), int(min_trim_size), int(extra_end_trim), float(end_threshold),
                                                start_trim.data_ptr(), end_trim.data_ptr(), nb, bs.ctypes.data, be.ctypes.data,
                                                float(barcode_threshold), float(barcode_diff), 1 if require_two else 0,
                                                call.data_ptr() if nb else None,
                                                traced_mask.data_ptr() if traced_mask is not None else None, ctypes.c_void_p(s)),
              "pc_phase_b_reduce")

    def phase_b_explain(self, records, n, job_record_offset, job_side, end_size, min_trim_size, extra_end_trim,
                        end_threshold, bins=None, traced_mask=None):
        """The per-read reasons behind phase_b_reduce (pc_phase_b_explain, both passes): same records, tables and
        conventions.  -> (summary int32[n, 12], bscore float64[n, 4], hit_first int64[n + 1], hits int32[total, 6]) CUDA
        tensors; the layout is documented in include/porechop_amd.h.  The prefix sum between the passes is a torch
        cumsum; its total is the call's one host round trip.  Everything -- both launches, the allocations, the cumsum --
        runs on torch's current stream, which is what orders the passes."""
        import torch
        assert records.is_cuda and records.dtype == torch.int32 and records.is_contiguous()
        n = int(n)
        dev = records.device
        off = np.ascontiguousarray(job_record_offset, dtype=np.int64)
        side = np.ascontiguousarray(job_side, dtype=np.int32)
        assert off.shape[0] == side.shape[0]
        if side.shape[0] and n:
            assert int(off.min()) >= 0 and int(off.max()) + n <= int(records.shape[0]), "job records outside the record tensor"
        nb = 0 if bins is None else len(bins)
        bs = np.ascontiguousarray([b[0] for b in bins] if nb else [0], dtype=np.int32)
        be = np.ascontiguousarray([b[1] for b in bins] if nb else [0], dtype=np.int32)
        if traced_mask is not None:
            assert traced_mask.is_cuda and traced_mask.dtype == torch.int64 and traced_mask.is_contiguous()
            assert tuple(traced_mask.shape) == (len(side), (n + 63) // 64)
        s = torch.cuda.current_stream().cuda_stream
        summary = torch.zeros((n, 12), dtype=torch.int32, device=dev)
        bscore = torch.zeros((n, 4), dtype=torch.float64, device=dev)
        hit_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)

        def launch(first, hits):
            check(self.lib.pc_phase_b_explain(self._ctx, records.data_ptr(), n, len(side), off.ctypes.data, side.ctypes.data,
                                              int(end_size), int(min_trim_size), int(extra_end_trim), float(end_threshold),
                                              nb, bs.ctypes.data, be.ctypes.data,
                                              traced_mask.data_ptr() if traced_mask is not None else None,
                                              summary.data_ptr(), bscore.data_ptr(), first.data_ptr() if first is not None else None,
                                              hits.data_ptr() if hits is not None else None, ctypes.c_void_p(s)),
                  "pc_phase_b_explain")
        launch(None, None)
        torch.cumsum(summary[:, 2].to(torch.int64) + summary[:, 3].to(torch.int64), 0, out=hit_first[1:])
        total = int(hit_first[-1].item()) if n else 0
        hits = torch.zeros((total, 6), dtype=torch.int32, device=dev)
        if total:
            launch(hit_first, hits)
        return summary, bscore, hit_first, hits

    def phase_b_select(self, records, n, job_off, job_side, job_len, job_calls, start_len, end_len, end_size, min_trim_size,
                       extra_end_trim, end_threshold, rnd, call_level, call_level_diff, mask_out, counts, mask_prev=None,
                       start_trim=None, end_trim=None, best_full=None, ub_trim_out=None, ub_full_out=None, stream=None):
        """Exact pruning of phase B, selection (pc_phase_b_select): all arguments CUDA tensors -- job_off int64[J],
        job_side / job_len / job_calls int32[J], start_len / end_len int32[n], mask_out / mask_prev int64[J, (n+63)//64],
        counts int64[J], best_full float64[2, n]."""
        import torch
        J = int(job_side.shape[0])
        assert records.dtype == torch.int32 and job_off.dtype == torch.int64 and mask_out.dtype == torch.int64 and counts.dtype == torch.int64
        assert job_side.dtype == job_len.dtype == job_calls.dtype == start_len.dtype == end_len.dtype == torch.int32
        assert tuple(mask_out.shape) == (J, (int(n) + 63) // 64) and mask_out.is_contiguous() and int(counts.shape[0]) == J
        ptr = lambda t: None if t is None else t.data_ptr()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_phase_b_select(self._ctx, records.data_ptr(), int(n), J, job_off.data_ptr(), job_side.data_ptr(),
                                         job_len.data_ptr(), job_calls.data_ptr(), start_len.data_ptr(), end_len.data_ptr(),
                                         int(end_size), int(min_trim_size), int(extra_end_trim), float(end_threshold), int(rnd),
                                         float(call_level), float(call_level_diff), ptr(mask_prev), ptr(start_trim), ptr(end_trim),
                                         ptr(best_full), mask_out.data_ptr(), counts.data_ptr(), ptr(ub_trim_out), ptr(ub_full_out),
                                         ctypes.c_void_p(s)), "pc_phase_b_select")

    def phase_b_gather(self, mask, n, job_first, cursor, job_off, job_side, start_off, start_len, end_off, end_len,
                       win_off, win_len, dest, pair_job, pair_read, stream=None):
        """The selected pairs as the window lists of a traced scan (pc_phase_b_gather)."""
        import torch
        J = int(job_side.shape[0])
        assert mask.dtype == torch.int64 and job_first.dtype == torch.int64 and cursor.dtype == torch.int64
        assert start_off.dtype == end_off.dtype == win_off.dtype == dest.dtype == pair_read.dtype == torch.int64
        assert start_len.dtype == end_len.dtype == win_len.dtype == pair_job.dtype == torch.int32
        assert start_off.is_contiguous() and end_off.is_contiguous() and start_len.is_contiguous() and end_len.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_phase_b_gather(self._ctx, mask.data_ptr(), int(n), J, job_first.data_ptr(), cursor.data_ptr(),
                                         job_off.data_ptr(), job_side.data_ptr(), start_off.data_ptr(), start_len.data_ptr(),
                                         end_off.data_ptr(), end_len.data_ptr(), win_off.data_ptr(), win_len.data_ptr(),
                                         dest.data_ptr(), pair_job.data_ptr(), pair_read.data_ptr(), ctypes.c_void_p(s)),
              "pc_phase_b_gather")

    def gather_records(self, records, index, out=None, stream=None):
        """out[k] = records[index[k]] on the device (pc_gather_records); records int32 [*, 8], index int64 [count]."""
        import torch
        assert records.dtype == torch.int32 and records.is_contiguous() and index.dtype == torch.int64 and index.is_contiguous()
        n = int(index.shape[0])
        if out is None:
            out = torch.empty((n, RESULT_INTS), dtype=torch.int32, device=records.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_gather_records(self._ctx, records.data_ptr(), index.data_ptr(), n, out.data_ptr(), ctypes.c_void_p(s)),
              "pc_gather_records")
        return out

    def phase_b_scatter(self, traced, dest, pair_job, pair_read, records, job_side, job_calls, best_full, n, stream=None):
        """Traced records over the score records they replace (pc_phase_b_scatter)."""
        import torch
        assert traced.dtype == torch.int32 and traced.is_contiguous() and records.dtype == torch.int32
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_phase_b_scatter(self._ctx, traced.data_ptr(), int(dest.shape[0]), dest.data_ptr(), pair_job.data_ptr(),
                                          pair_read.data_ptr(), records.data_ptr(), job_side.data_ptr(), job_calls.data_ptr(),
                                          None if best_full is None else best_full.data_ptr(), int(n), ctypes.c_void_p(s)),
              "pc_phase_b_scatter")

    def copy_windows(self, arena, src_off, length, dst, dst_off, pad, stream=None):
        """Packed private copies on the device (pc_copy_windows): window i of `arena` -> dst[dst_off[i]:], padded
        with `pad` up to dst_off[i+1]; src_off int64[n], length int32[n], dst_off int64[n+1], all CUDA tensors."""
        import torch
        n = int(src_off.shape[0])
        assert arena.is_cuda and dst.is_cuda and src_off.dtype == torch.int64 and length.dtype == torch.int32
        assert dst_off.dtype == torch.int64 and int(dst_off.shape[0]) == n + 1
        assert src_off.is_contiguous() and length.is_contiguous() and dst_off.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_copy_windows(self._ctx, arena.data_ptr(), src_off.data_ptr(), length.data_ptr(), n, dst.data_ptr(),
                                       dst_off.data_ptr(), int(pad), ctypes.c_void_p(s)), "pc_copy_windows")

    def unpack_device(self, packed, nbases, exceptions, arena=None, pad=64, stream=None):
        """2 bits per base -> the byte arena the scans take, on the device (pc_unpack_device).  packed: uint8 CUDA tensor
        (io.pack_reads' plane, uploaded); exceptions: int64 CUDA tensor of the non-ACGT positions; arena: optional
        preallocated uint8 CUDA tensor of >= nbases + pad bytes.  -> the arena (nbases bases + `pad` bytes of 'N')."""
        import torch
        assert packed.is_cuda and packed.dtype == torch.uint8 and packed.is_contiguous()
        nbases = int(nbases)
        assert int(packed.numel()) * 4 >= nbases
        if arena is None:
            arena = torch.empty(nbases + pad, dtype=torch.uint8, device=packed.device)
        assert arena.is_cuda and arena.dtype == torch.uint8 and int(arena.numel()) >= nbases + pad
        ne = 0 if exceptions is None else int(exceptions.numel())
        if ne:
            assert exceptions.is_cuda and exceptions.dtype == torch.int64 and exceptions.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_unpack_device(self._ctx, packed.data_ptr(), nbases, exceptions.data_ptr() if ne else None, ne,
                                        arena.data_ptr(), int(pad), ctypes.c_void_p(s)), "pc_unpack_device")
        return arena

    def max_edits(self, adapter_len, threshold_percent):
        """Most non-matching columns an alignment of an adapter_len-base adapter can have inside the adapter's span if
        its full-adapter identity reaches threshold_percent (pc_prefilter_max_edits)."""
        return int(self.lib.pc_prefilter_max_edits(int(adapter_len), float(threshold_percent)))

    def prefilter_mask(self, arena, win_off, win_len, max_len, adapters, max_edits, stream=None):
        """Exact prefilter (pc_prefilter_device) -> int32 CUDA tensor [n, ceil(len(adapters) / 32)]: bit j % 32 of word
        j // 32 of row w is clear when window w is PROVEN not to hold adapters[j] within max_edits[j] edits."""
        import torch
        assert arena.is_cuda and win_off.is_cuda and win_len.is_cuda
        assert win_off.dtype == torch.int64 and win_len.dtype == torch.int32 and win_off.is_contiguous() and win_len.is_contiguous()
        n, na = int(win_off.shape[0]), len(adapters)
        words = (na + 31) // 32
        mask = torch.empty((n, max(words, 1)), dtype=torch.int32, device=arena.device)
        if na == 0:
            return mask.zero_()
        ad = np.ascontiguousarray(adapters, dtype=np.int32)
        ed = np.ascontiguousarray(max_edits, dtype=np.int32)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_prefilter_device(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n, int(max_len),
                                           ad.ctypes.data, ed.ctypes.data, na, mask.data_ptr(), ctypes.c_void_p(s)),
              "pc_prefilter_device")
        return mask

    def prefilter_mask_packed(self, plane, win_off, win_len, max_len, adapters, max_edits, stream=None, total=False):
        """prefilter_mask over reads held at 2 bits per base (pc_prefilter_packed): plane = the uint8 CUDA tensor of
        io.pack_reads' plane (64 readable bytes past the last base), win_off in BASES.  -> the mask, or None when this
        adapter list does not take the packed route (an adapter with a letter other than A/C/G/T/U, or one the seed stage
        cannot cover): unpack and call prefilter_mask.
        total=True (pc_prefilter_packed_any): every list is taken -- what the seed stage cannot cover runs the exhaustive
        kernel over the plane, adapter letters that are not bases as wildcards -- and None is never returned."""
        import torch
        assert plane.is_cuda and plane.dtype == torch.uint8 and win_off.is_cuda and win_len.is_cuda
        assert win_off.dtype == torch.int64 and win_len.dtype == torch.int32 and win_off.is_contiguous() and win_len.is_contiguous()
        n, na = int(win_off.shape[0]), len(adapters)
        words = (na + 31) // 32
        mask = torch.empty((n, max(words, 1)), dtype=torch.int32, device=plane.device)
        if na == 0:
            return mask.zero_()
        ad = np.ascontiguousarray(adapters, dtype=np.int32)
        ed = np.ascontiguousarray(max_edits, dtype=np.int32)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if total:
            check(self.lib.pc_prefilter_packed_any(self._ctx, plane.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n, int(max_len),
                                                   ad.ctypes.data, ed.ctypes.data, na, mask.data_ptr(), ctypes.c_void_p(s)),
                  "pc_prefilter_packed_any")
            return mask
        rc = self.lib.pc_prefilter_packed(self._ctx, plane.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), n, int(max_len),
                                          ad.ctypes.data, ed.ctypes.data, na, mask.data_ptr(), ctypes.c_void_p(s))
        if rc == -2:                              # PC_ERR_UNSUPPORTED_SCORES: not a list for the packed route
            return None
        check(rc, "pc_prefilter_packed")
        return mask

    def unpack_windows(self, plane, exceptions, src_off, length, dst, dst_off, pad=ord("N"), stream=None):
        """Windows of the 2-bit plane as bytes (pc_unpack_windows): src_off int64[n] in bases (ascending, not overlapping),
        length int32[n], dst uint8, dst_off int64[n + 1]; 'N' at the listed exceptions (int64, ascending; may be None)."""
        import torch
        n = int(src_off.shape[0])
        assert plane.is_cuda and dst.is_cuda and src_off.dtype == torch.int64 and length.dtype == torch.int32
        assert dst_off.dtype == torch.int64 and int(dst_off.shape[0]) == n + 1
        assert src_off.is_contiguous() and length.is_contiguous() and dst_off.is_contiguous()
        ne = 0 if exceptions is None else int(exceptions.numel())
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_unpack_windows(self._ctx, plane.data_ptr(), exceptions.data_ptr() if ne else None, ne, src_off.data_ptr(),
                                         length.data_ptr(), n, dst.data_ptr(), dst_off.data_ptr(), int(pad), ctypes.c_void_p(s)),
              "pc_unpack_windows")
        return dst

    # ---- the glue of the middle scan as single launches (pc_middle.hip).  middle.TorchGlue is the same contract in torch
    # expressions, for aligners without them (the test stand-ins); middle.choose_glue picks one per call
    STAT_BIG = 1 << 40

    def trim_windows(self, off, length, start_trim, end_trim):
        """-> (toff int64[R], tlen int32[R], stats int64[4] on the device: live, longest, STAT_BIG - shortest non-empty, sum)"""
        import torch
        n = int(off.shape[0])
        toff = torch.empty(n, dtype=torch.int64, device=off.device)
        tlen = torch.empty(n, dtype=torch.int32, device=off.device)
        stats = torch.empty(4, dtype=torch.int64, device=off.device)
        off, length = off.contiguous(), length.contiguous()
        st, et = start_trim.to(torch.int32).contiguous(), end_trim.to(torch.int32).contiguous()
        assert off.dtype == torch.int64 and length.dtype == torch.int32
        s = torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_trim_windows(self._ctx, off.data_ptr(), length.data_ptr(), st.data_ptr(), et.data_ptr(), n, toff.data_ptr(),
                                       tlen.data_ptr(), stats.data_ptr(), ctypes.c_void_p(s)), "pc_trim_windows")
        return toff, tlen, stats

    def middle_hits(self, rec, threshold):
        """rec int32[..., 8] (contiguous) -> (full float64[...], hit bool[...])"""
        import torch
        assert rec.dtype == torch.int32 and rec.is_contiguous() and rec.shape[-1] == RESULT_INTS
        shape = rec.shape[:-1]
        n = int(rec.numel() // RESULT_INTS)
        full = torch.empty(shape, dtype=torch.float64, device=rec.device)
        hit = torch.empty(shape, dtype=torch.uint8, device=rec.device)
        s = torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_middle_hits(self._ctx, rec.data_ptr(), n, float(threshold), full.data_ptr(), hit.data_ptr(), ctypes.c_void_p(s)),
              "pc_middle_hits")
        return full, hit.view(torch.bool)

    def group_survivors(self, mask, gmask):
        """mask int32[n, words], gmask int32[G, words] (device) -> (cand bool[G, n], counts int64[G] on the device)"""
        import torch
        n, words = int(mask.shape[0]), int(mask.shape[1])
        G = int(gmask.shape[0])
        assert mask.dtype == torch.int32 and mask.is_contiguous() and gmask.dtype == torch.int32 and gmask.is_contiguous() and int(gmask.shape[1]) == words
        cand = torch.empty((G, n), dtype=torch.uint8, device=mask.device)
        counts = torch.empty(G, dtype=torch.int64, device=mask.device)
        s = torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_group_survivors(self._ctx, mask.data_ptr(), n, words, gmask.data_ptr(), G, cand.data_ptr(), counts.data_ptr(),
                                          ctypes.c_void_p(s)), "pc_group_survivors")
        return cand.view(torch.bool), counts

    def round_consume(self, full_all, rec_all, cur, act, threshold):
        """One consuming step of mask-and-realign (pc_round_consume) -> (anyh bool[n], a_hit int32[n], cnt int64[n], stats int64[4])"""
        import torch
        A, Dn = int(full_all.shape[0]), int(full_all.shape[1])
        n = int(act.shape[0])
        assert full_all.dtype == torch.float64 and full_all.is_contiguous() and rec_all.dtype == torch.int32 and rec_all.is_contiguous()
        assert cur.dtype == torch.int64 and cur.is_contiguous() and act.dtype == torch.int64
        act = act.contiguous()
        anyh = torch.empty(n, dtype=torch.uint8, device=act.device)
        a_hit = torch.empty(n, dtype=torch.int32, device=act.device)
        cnt = torch.empty(n, dtype=torch.int64, device=act.device)
        stats = torch.empty(4, dtype=torch.int64, device=act.device)
        s = torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_round_consume(self._ctx, full_all.data_ptr(), rec_all.data_ptr(), cur.data_ptr(), act.data_ptr(), n, A, Dn, float(threshold),
                                        anyh.data_ptr(), a_hit.data_ptr(), cnt.data_ptr(), stats.data_ptr(), ctypes.c_void_p(s)), "pc_round_consume")
        return anyh.view(torch.bool), a_hit, cnt, stats

    def round_consume_select(self, full_all, rec_all, cur, act, threshold, set_of, nsets, floored_positive):
        """round_consume and, behind it, which adapter sets the next round must scan for which of the reads that hit
        (pc_round_select, csrc/pc_mask_rule.h) -> (anyh, a_hit, cnt, stats int64[4 + nsets], need uint8[nsets, n]): the
        four statistics and the per-set counts in ONE buffer, for one copy to the host.  set_of int32[A] on the device."""
        import torch
        A, Dn = int(full_all.shape[0]), int(full_all.shape[1])
        n = int(act.shape[0])
        assert full_all.dtype == torch.float64 and full_all.is_contiguous() and rec_all.dtype == torch.int32 and rec_all.is_contiguous()
        assert cur.dtype == torch.int64 and cur.is_contiguous() and act.dtype == torch.int64
        assert set_of.dtype == torch.int32 and set_of.is_contiguous() and int(set_of.shape[0]) == A and nsets >= 1
        act = act.contiguous()
        dev = act.device
        anyh = torch.empty(n, dtype=torch.uint8, device=dev)
        a_hit = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int64, device=dev)
        stats = torch.empty(4 + nsets, dtype=torch.int64, device=dev)
        need = torch.empty((nsets, n), dtype=torch.uint8, device=dev)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self.lib.pc_round_consume(self._ctx, full_all.data_ptr(), rec_all.data_ptr(), cur.data_ptr(), act.data_ptr(), n, A, Dn, float(threshold),
                                        anyh.data_ptr(), a_hit.data_ptr(), cnt.data_ptr(), stats.data_ptr(), s), "pc_round_consume")
        check(self.lib.pc_round_select(self._ctx, rec_all.data_ptr(), act.data_ptr(), anyh.data_ptr(), a_hit.data_ptr(), set_of.data_ptr(), n, A, Dn,
                                       int(nsets), 1 if floored_positive else 0, need.data_ptr(), stats.data_ptr() + 32, s), "pc_round_select")
        return anyh.view(torch.bool), a_hit, cnt, stats, need

    def prefilter_defer_count(self, enabled=True):
        """No host round trip inside prefilter_mask (pc_prefilter_defer_count): after the caller's next synchronisation,
        prefilter_overflowed() says whether the last mask is incomplete (then: call again with the deferral off)."""
        check(self.lib.pc_prefilter_defer_count(self._ctx, 1 if enabled else 0), "pc_prefilter_defer_count")

    def prefilter_overflowed(self):
        return bool(self.lib.pc_prefilter_overflowed(self._ctx))

    def prefilter_rows(self, arena, win_off, win_len, max_len, adapters, max_edits, stream=None, packed=False, total=False):
        """The prefilter's survivors, sparsely: -> (rows int64 [R]: the windows with at least one surviving adapter, in
        increasing order; bits bool [R, len(adapters)]: which).  Everything not listed is PROVEN not to be a hit."""
        import torch
        if packed:              # arena is the 2-bit plane, win_off counts bases; None = this list does not take the packed route
            mask = self.prefilter_mask_packed(arena, win_off, win_len, max_len, adapters, max_edits, stream, total=total)   # (total: never None)
            if mask is None:
                return None
        else:
            mask = self.prefilter_mask(arena, win_off, win_len, max_len, adapters, max_edits, stream)
        na = len(adapters)
        rows = torch.nonzero((mask != 0).any(dim=1)).flatten()
        sub = mask[rows]
        shifts = torch.arange(32, device=mask.device, dtype=torch.int32)
        bits = ((sub[:, :, None] >> shifts[None, None, :]) & 1).reshape(int(rows.shape[0]), 32 * int(mask.shape[1]))[:, :na].to(torch.bool)
        return rows, bits

    def prefilter(self, arena, win_off, win_len, max_len, adapters, max_edits, stream=None):
        """Dense form of prefilter_rows: bool CUDA tensor [len(adapters), n] (small batches, tests)."""
        import torch
        rows, bits = self.prefilter_rows(arena, win_off, win_len, max_len, adapters, max_edits, stream)
        out = torch.zeros((len(adapters), int(win_off.shape[0])), dtype=torch.bool, device=arena.device)
        out[:, rows] = bits.t()
        return out

    # ---- adapter discovery: the k-mer census (pc_discover.hip) --------------------------------------------------------
    def kmer_count(self, arena, win_off, win_len, k, counts=None, stream=None):
        """counts[code] += 1 for every k-mer of the n windows (pc_kmer_count: 2 bits per base, first base highest, A C G T/U
        = 0 1 2 3, k-mers over any other byte skipped).  arena uint8, win_off int64[n], win_len int32[n]: CUDA tensors;
        counts: the int32 CUDA tensor [4^k] to add to (its bits are the library's uint32 counters), or None for a zeroed
        one.  -> counts.  Asynchronous."""
        import torch
        k = int(k)
        assert arena.is_cuda and arena.dtype == torch.uint8 and win_off.dtype == torch.int64 and win_len.dtype == torch.int32
        assert win_off.is_contiguous() and win_len.is_contiguous() and win_off.shape[0] == win_len.shape[0]
        if counts is None and 4 <= k <= 13:
            counts = torch.zeros(1 << (2 * k), dtype=torch.int32, device=arena.device)
        if counts is not None:
            assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and int(counts.numel()) == 1 << (2 * k)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_kmer_count(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), int(win_off.shape[0]), k,
                                     None if counts is None else counts.data_ptr(), ctypes.c_void_p(s)), "pc_kmer_count")
        return counts

    def kmer_select(self, counts, k, min_count, cap, stream=None):
        """The raw pc_kmer_select: -> (codes int32[cap], cnt int32[cap], found int64[1]) on the device.  The first
        min(found, cap) entries are table entries with count >= min_count, in no particular order; found counts all of them."""
        import torch
        cap = int(cap)
        codes = torch.empty(cap, dtype=torch.int32, device=counts.device)
        cnt = torch.empty(cap, dtype=torch.int32, device=counts.device)
        found = torch.empty(1, dtype=torch.int64, device=counts.device)
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_kmer_select(self._ctx, counts.data_ptr(), int(k), int(min_count), codes.data_ptr() if cap else None,
                                      cnt.data_ptr() if cap else None, cap, found.data_ptr(), ctypes.c_void_p(s)), "pc_kmer_select")
        return codes, cnt, found

    def kmer_candidates(self, counts, k, min_count, cap=1 << 16):
        """The k-mers seen at least min_count times -> (codes int64[m], counts int64[m]) as numpy arrays, sorted by count
        descending, then code ascending.  `cap` sizes the first list; an overflow is retried with the size the cursor reported."""
        assert int(counts.numel()) == 1 << (2 * int(k))
        while True:
            codes, cnt, found = self.kmer_select(counts, k, min_count, cap)
            m = int(found.item())                           # (synchronises)
            if m <= cap:
                break
            cap = m
        codes = codes[:m].cpu().numpy().astype(np.int64)
        cnt = cnt[:m].cpu().numpy().view(np.uint32).astype(np.int64)
        order = np.lexsort((codes, -cnt))
        return codes[order], cnt[order]

    def anchor_inserts(self, arena, win_off, win_len, records, anchor_len, side, min_identity=75, insert_len=24, stream=None):
        """The insert_len bases right behind (side 0: start windows) or before (side 1: end windows) an anchor's alignment in
        each of the n windows, as one 2-bit code per window (pc_anchor_inserts: the first base in the highest bits; -1 where the
        window is not anchored, the insert does not fit the window or holds a byte that is not a base).  records int32[n, 8]:
        the scan records of the anchor (anchor_len bases) against these windows, window order; arena uint8, win_off int64[n],
        win_len int32[n]: CUDA tensors.  min_identity 0..100 (an integer: matches * 100 >= min_identity * full length).
        -> int64 CUDA tensor [n].  Asynchronous."""
        import torch
        n = int(win_off.shape[0])
        assert arena.is_cuda and arena.dtype == torch.uint8 and win_off.dtype == torch.int64 and win_len.dtype == torch.int32
        assert records.is_cuda and records.dtype == torch.int32 and records.is_contiguous() and int(records.numel()) == n * RESULT_INTS
        assert win_off.is_contiguous() and win_len.is_contiguous() and int(win_len.shape[0]) == n
        codes = torch.empty(n, dtype=torch.int64, device=arena.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_anchor_inserts(self._ctx, arena.data_ptr(), win_off.data_ptr(), win_len.data_ptr(), records.data_ptr(), n,
                                         int(anchor_len), int(side), int(min_identity), int(insert_len), codes.data_ptr(),
                                         ctypes.c_void_p(s)), "pc_anchor_inserts")
        return codes

    def debug_value_range(self):
        """(lo, hi) of the DP values the range-checking kernel builds have held since the last call."""
        lo, hi = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.pc_debug_value_range(self._ctx, ctypes.byref(lo), ctypes.byref(hi)), "pc_debug_value_range")
        return lo.value, hi.value

    def trace_ops_per_2_cells(self):
        """Packed VALU ops the traced end-window kernel spends per two DP cells (roofline reporting)."""
        return self.lib.pc_trace_ops_x100(self._ctx) / 100.0

    def sync(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.lib.pc_sync(self._ctx, ctypes.c_void_p(s)), "pc_sync")
