"""TEST INFRASTRUCTURE: an independent restatement of one adapter alignment under the IUPAC-wildcard rule, in plain
Python / numpy, written from SURVEY.md section 8a (recurrence a-2, scout a-3, traceback a-4, digest a-5, all read literally:
full trace bytes, gapped rows) and from the rule of DESIGN.md section 15.  It binds to nothing under test: not to the library,
not to pc_cell.h / pc_walk.h / pc_letters.h, not to the oracle.  The linear dispatch (gap_open == gap_extend), which the survey
does not restate, is the one the goldens record: S = diagonal; strict '<' against vertical, then against horizontal; every gap
step a step of its own.

    align_many(pairs, scores, wildcards=True) -> (records int32 [n, 8], paths)

records are the library's eight integers (read_start, read_end, adapter_start, adapter_end, score, matches, aligned_len,
full_len); paths[k] = (read_first, adapter_first, cigar) with the FORWARD run-length string over = X I D ('=' a diagonal step
that matches under the rule, 'X' one that does not, 'I' a read base against a gap, 'D' an adapter base against a gap).

The DP runs over anti-diagonals for a whole batch of pairs at once (numpy); scout, traceback and digest run per pair.
wildcards=False is the reference's own equality of Dna5 codes (N == N), which anchors this file to the committed goldens."""
import numpy as np

INT_MIN = -2 ** 31
NEG_INF = INT_MIN // 2

# trace bits, seqan/align/dp_profile.h:142-156
NONE, DIAGONAL, HORIZONTAL, VERTICAL, HORIZONTAL_OPEN, VERTICAL_OPEN, MAX_FROM_HORIZONTAL, MAX_FROM_VERTICAL = 0, 1, 2, 4, 8, 16, 32, 64

_A, _C, _G, _T = 1, 2, 4, 8
IUPAC = {"A": _A, "C": _C, "G": _G, "T": _T, "U": _T,
         "R": _A | _G, "Y": _C | _T, "S": _C | _G, "W": _A | _T, "K": _G | _T, "M": _A | _C,
         "B": _C | _G | _T, "D": _A | _G | _T, "H": _A | _C | _T, "V": _A | _C | _G, "N": _A | _C | _G | _T}


def read_code(byte):
    """Dna5: A 0, C 1, G 2, T / U 3 (either case), everything else 4."""
    return {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}.get(chr(byte).upper(), 4)


def letter_set(byte, wildcards):
    """The set of read codes (bit k = code k) an adapter byte matches."""
    if wildcards:
        return IUPAC.get(chr(byte).upper(), 0)           # bit 4 never set; any other byte: the empty set
    return 1 << read_code(byte)                          # the reference: equal Dna5 codes, N == N


def first_member(byte):
    """The first base (in the order A, C, G, T) of an adapter letter's wildcard set, or None for the empty set."""
    s = letter_set(byte, True)
    for k, ch in enumerate("ACGT"):
        if s >> k & 1:
            return ch
    return None


_RC = np.array([read_code(b) for b in range(256)], dtype=np.int64)


def _bytes(x):
    return x if isinstance(x, (bytes, bytearray)) else x.encode()


def _dp_batch(reads, adapters, schemes, wildcards):
    """Full M, H, V and trace matrices of a batch: arrays [B, nmax + 1, mmax + 1] (column j, row i)."""
    B = len(reads)
    n = np.array([len(r) for r in reads])
    m = np.array([len(a) for a in adapters])
    nmax, mmax = int(n.max()), int(m.max())
    rc = np.full((B, nmax + 1), 4, dtype=np.int64)          # rc[b, j]: code of read base j (1-based)
    st = np.zeros((B, mmax + 1), dtype=np.int64)            # st[b, i]: set of adapter letter i (1-based)
    for b in range(B):
        rc[b, 1:n[b] + 1] = _RC[np.frombuffer(reads[b], dtype=np.uint8)]
        st[b, 1:m[b] + 1] = [letter_set(x, wildcards) for x in adapters[b]]
    sc = np.array(schemes, dtype=np.int64).reshape(B, 4)
    ma, mi, go, ge = (sc[:, k:k + 1] for k in range(4))
    lin = go == ge
    Mf = np.zeros((B, nmax + 1, mmax + 1), dtype=np.int64)
    Hf = np.full((B, nmax + 1, mmax + 1), NEG_INF, dtype=np.int64)
    Vf = np.full((B, nmax + 1, mmax + 1), NEG_INF, dtype=np.int64)
    Tf = np.zeros((B, nmax + 1, mmax + 1), dtype=np.uint8)
    i = np.arange(1, mmax + 1)
    zeros = np.zeros((B, mmax + 1), dtype=np.int64)
    negs = np.full((B, mmax + 1), NEG_INF, dtype=np.int64)
    p2 = (zeros, negs, negs)                                 # diagonal d - 2, indexed by row: (M, H, V)
    p1 = (zeros, negs, negs)                                 # diagonal d - 1
    for d in range(2, nmax + mmax + 1):
        j = d - i
        valid = (j >= 1) & (j <= nmax)
        if not valid.any():
            continue
        jc = np.clip(j, 0, nmax)
        m_left, h_left = p1[0][:, 1:], p1[1][:, 1:]          # (i, j - 1)
        m_up, v_up = p1[0][:, :-1], p1[2][:, :-1]            # (i - 1, j)
        m_diag = p2[0][:, :-1]                               # (i - 1, j - 1)
        sub = np.where((st[:, 1:] >> rc[:, jc]) & 1, ma, mi)
        dd = m_diag + sub
        # affine (a-2, comparisons as written)
        hs = h_left + ge
        t = m_left + go
        c = hs < t
        hs = np.where(c, t, hs)
        g = np.where(c, HORIZONTAL_OPEN, HORIZONTAL)
        vs = v_up + ge
        t = m_up + go
        c = vs < t
        vs = np.where(c, t, vs)
        g = g | np.where(c, VERTICAL_OPEN, VERTICAL)
        s = vs
        c = s < hs
        s = np.where(c, hs, s)
        mx = np.where(c, MAX_FROM_HORIZONTAL, MAX_FROM_VERTICAL)
        c = s <= dd
        s = np.where(c, dd, s)
        tr = np.where(c, DIAGONAL | g, g | mx)
        # linear: diagonal, then strict '<' against vertical, then against horizontal; every gap step on its own
        sl = dd
        tl = np.full_like(tr, DIAGONAL)
        t = m_up + ge
        c = sl < t
        sl = np.where(c, t, sl)
        tl = np.where(c, MAX_FROM_VERTICAL | VERTICAL_OPEN, tl)
        t = m_left + ge
        c = sl < t
        sl = np.where(c, t, sl)
        tl = np.where(c, MAX_FROM_HORIZONTAL | HORIZONTAL_OPEN, tl)
        s = np.where(lin, sl, s)
        hs = np.where(lin, NEG_INF, hs)
        vs = np.where(lin, NEG_INF, vs)
        tr = np.where(lin, tl, tr)
        nm, nh, nv = zeros.copy(), negs.copy(), negs.copy()
        nm[:, 1:] = np.where(valid, s, 0)
        nh[:, 1:] = np.where(valid, hs, NEG_INF)
        nv[:, 1:] = np.where(valid, vs, NEG_INF)
        iv, jv = i[valid], j[valid]
        Mf[:, jv, iv] = s[:, valid]
        Hf[:, jv, iv] = hs[:, valid]
        Vf[:, jv, iv] = vs[:, valid]
        Tf[:, jv, iv] = tr[:, valid]
        p2, p1 = p1, (nm, nh, nv)
    return Mf, Hf, Vf, Tf


def _finish_pair(read, adapter, M, H, V, T, wildcards):
    """Scout (a-3), traceback (a-4) and digest (a-5) of one pair from its matrices [n + 1, m + 1]."""
    n, m = len(read), len(adapter)
    # a-3: (m, 0), then (m, j) for j = 1 .. n - 1, then the last column top to bottom; strict '>': the earliest maximum
    cand = [(m, 0)] + [(m, j) for j in range(1, n)] + [(i, n) for i in range(0, m + 1)]
    vals = np.array([0] + [M[j, m] for j in range(1, n)] + [M[n, i] for i in range(0, m + 1)])
    I, J = cand[int(np.argmax(vals))]
    score = int(vals.max())
    bM, bH, bV = (int(M[J, I]), int(H[J, I]), int(V[J, I])) if (I > 0 and J > 0) else (0, NEG_INF, NEG_INF)
    tr = T.tolist()
    tv = tr[J][I] if (I > 0 and J > 0) else NONE
    if bV == bM:
        tv = (tv & ~DIAGONAL) | MAX_FROM_VERTICAL
    elif bH == bM:
        tv = (tv & ~DIAGONAL) | MAX_FROM_HORIZONTAL
    if tv & MAX_FROM_VERTICAL:
        tv &= VERTICAL | VERTICAL_OPEN | MAX_FROM_VERTICAL
        last = VERTICAL
    elif tv & MAX_FROM_HORIZONTAL:
        tv &= HORIZONTAL | HORIZONTAL_OPEN | MAX_FROM_HORIZONTAL
        last = HORIZONTAL
    else:
        last = DIAGONAL
    col, row, frag = J, I, 0
    tail, path, head = [], [], []

    def emit(where, kind, ln):
        if ln:
            where.append(("D" if kind & DIAGONAL else "V" if kind & VERTICAL else "H", ln))

    def at(c, r):
        return tr[c][r] if (c > 0 and r > 0) else NONE

    if row != m:
        emit(tail, VERTICAL, m - row)
    if col != n:
        emit(tail, HORIZONTAL, n - col)
    while col > 0 and row > 0 and tv != NONE:
        if tv & DIAGONAL:
            if not last & DIAGONAL:
                emit(path, last, frag)
                last, frag = DIAGONAL, 0
            col -= 1
            row -= 1
            tv = at(col, row)
            frag += 1
        elif tv & MAX_FROM_VERTICAL and tv & VERTICAL:
            if not last & VERTICAL:
                emit(path, last, frag)
                last, frag = VERTICAL, 0
            while (not tv & VERTICAL_OPEN or tv & VERTICAL) and row != 1:
                row -= 1
                tv = at(col, row)
                frag += 1
            row -= 1
            tv = at(col, row)
            frag += 1
        elif tv & MAX_FROM_VERTICAL and tv & VERTICAL_OPEN:
            if not last & VERTICAL:
                emit(path, last, frag)
                last, frag = VERTICAL, 0
            row -= 1
            tv = at(col, row)
            frag += 1
        elif tv & MAX_FROM_HORIZONTAL and tv & HORIZONTAL:
            if not last & HORIZONTAL:
                emit(path, last, frag)
                last, frag = HORIZONTAL, 0
            while (not tv & HORIZONTAL_OPEN or tv & HORIZONTAL) and col != 1:
                col -= 1
                tv = at(col, row)
                frag += 1
            col -= 1
            tv = at(col, row)
            frag += 1
        elif tv & MAX_FROM_HORIZONTAL and tv & HORIZONTAL_OPEN:
            if not last & HORIZONTAL:
                emit(path, last, frag)
                last, frag = HORIZONTAL, 0
            col -= 1
            tv = at(col, row)
            frag += 1
        else:
            raise AssertionError("trace byte %d has no direction" % tv)
    emit(path, last, frag)
    read_first, adapter_first = col, row
    if row != 0:
        emit(head, VERTICAL, row)
    if col != 0:
        emit(head, HORIZONTAL, col)
    # the gapped rows, left to right: per column (read base index or None, adapter base index or None)
    columns = []
    rb = ab = 0
    for kind, ln in list(reversed(head)) + list(reversed(path)) + list(reversed(tail)):
        for _ in range(ln):
            if kind == "D":
                columns.append((rb, ab)); rb += 1; ab += 1
            elif kind == "H":
                columns.append((rb, None)); rb += 1
            else:
                columns.append((None, ab)); ab += 1
    assert rb == n and ab == m, (rb, n, ab, m)

    def equal(c):
        return c[0] is not None and c[1] is not None and bool(letter_set(adapter[c[1]], wildcards) >> read_code(read[c[0]]) & 1)

    # a-5
    L = len(columns)
    start = end = None
    rs = as_ = False
    for k in range(L):
        rs |= columns[k][0] is not None
        as_ |= columns[k][1] is not None
        if rs and as_:
            start = k
            break
    rs = as_ = False
    for k in range(L - 1, -1, -1):
        rs |= columns[k][0] is not None
        as_ |= columns[k][1] is not None
        if rs and as_:
            end = k
            break
    a_cols = [k for k in range(L) if columns[k][1] is not None]
    a_start, a_end = a_cols[0], a_cols[-1]
    am = sum(equal(columns[k]) for k in range(start, end + 1))
    fm = sum(equal(columns[k]) for k in range(a_start, a_end + 1))
    assert am == fm, (am, fm)
    consumed = lambda k, side: sum(c[side] is not None for c in columns[:k])
    rec = (consumed(start, 0), consumed(end, 0), consumed(start, 1), consumed(end, 1), score, am, max(0, end - start + 1), a_end - a_start + 1)
    # the path's operations, forward
    ops = []
    rb, ab = read_first, adapter_first
    for kind, ln in reversed(path):
        for _ in range(ln):
            if kind == "D":
                ops.append("=" if equal((rb, ab)) else "X"); rb += 1; ab += 1
            elif kind == "H":
                ops.append("I"); rb += 1
            else:
                ops.append("D"); ab += 1
    assert (rb, ab) == (J, I)
    return rec, (read_first, adapter_first, run_lengths(ops)), (J, I)


def run_lengths(ops):
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append("%d%s" % (e - k, ops[k]))
        k = e
    return "".join(out)


def expand(cigar):
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.extend(ch * int(num))
            num = ""
    return out


def align_many(pairs, scores=(3, -6, -5, -2), wildcards=True, batch=96, cells=None):
    """pairs: [(read, adapter)] (str or bytes); scores: one scheme for all, or one per pair.  cells: a list that receives the
    scout's end cell (column, row) of every pair, (0, 0) for an empty read or adapter."""
    pairs = [(_bytes(r), _bytes(a)) for r, a in pairs]
    N = len(pairs)
    schemes = [tuple(scores)] * N if np.ndim(scores) == 1 else [tuple(s) for s in scores]
    records = np.zeros((N, 8), dtype=np.int32)
    paths = [None] * N
    ends = [(0, 0)] * N
    live = []
    for k, (r, a) in enumerate(pairs):
        if len(r) == 0 or len(a) == 0:                 # alignment.cpp:9-21: only field 0 and the score are defined
            records[k] = (-1, 0, -1, 0, INT_MIN, 0, 0, 0)
            paths[k] = (0, 0, "")
        else:
            live.append(k)
    live.sort(key=lambda k: (len(pairs[k][1]), len(pairs[k][0])))      # similar shapes together: little padding
    for lo in range(0, len(live), batch):
        ks = live[lo:lo + batch]
        Mf, Hf, Vf, Tf = _dp_batch([pairs[k][0] for k in ks], [pairs[k][1] for k in ks], [schemes[k] for k in ks], wildcards)
        for b, k in enumerate(ks):
            n, m = len(pairs[k][0]), len(pairs[k][1])
            rec, path, ends[k] = _finish_pair(pairs[k][0], pairs[k][1], Mf[b, :n + 1, :m + 1], Hf[b, :n + 1, :m + 1], Vf[b, :n + 1, :m + 1],
                                     Tf[b, :n + 1, :m + 1], wildcards)
            records[k] = rec
            paths[k] = path
    if cells is not None:
        cells[:] = ends
    return records, paths


def align(read, adapter, scores=(3, -6, -5, -2), wildcards=True):
    rec, paths = align_many([(read, adapter)], scores, wildcards)
    return rec[0], paths[0]


def format_record(rec):
    """The reference's seven-field string (alignment.cpp:113-121: %d and %f)."""
    rs, re_, as_, ae, score, m, al, fl = (int(x) for x in rec)
    partial = "-nan" if al == 0 else "%f" % (100.0 * m / al)
    full = "%f" % (100.0 * m / fl) if fl else "-nan"
    return "%d,%d,%d,%d,%d,%s,%s" % (rs, re_, as_, ae, score, partial, full)


def rescore(read, adapter, path, wildcards=True):
    """A path replayed under the rule -> (matches, diagonal steps, gap steps, ok): ok says that every '=' sits on a match and
    every 'X' on a diagonal step that is none.  With the path's `opens` (gap steps that opened their gap) its score is
    match * matches + mismatch * (diagonal - matches) + gap_open * opens + gap_extend * (gaps - opens)."""
    read, adapter = _bytes(read), _bytes(adapter)
    rb, ab, cigar = path
    matches = diag = gaps = 0
    ok = True
    for op in expand(cigar):
        if op in "=X":
            match = bool(letter_set(adapter[ab], wildcards) >> read_code(read[rb]) & 1)
            ok &= match == (op == "=")
            matches += match
            diag += 1
            rb += 1
            ab += 1
        elif op == "I":
            gaps += 1
            rb += 1
        else:
            gaps += 1
            ab += 1
    return matches, diag, gaps, ok
