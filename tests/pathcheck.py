"""What a returned alignment path has to satisfy, in plain Python (TEST INFRASTRUCTURE; no GPU).

check_path() takes one pair -- read window, adapter, scheme -- with the record, head and FORWARD operation string the
library returned for it and the oracle's result, and asserts the per-pair properties of tests/host/test_paths.cpp:
  (b) the operations, replayed from (adapter_first, read_first), stay inside the rectangle, every '=' on equal Dna5 codes
      (N == N is equal) and every 'X' on unequal ones;
  (c) the replay ends in the last row or the last column, at the oracle's end cell;
  (d) read_first + adapter_first + path_len + (n - end_j) + (m - end_i) is the oracle's path length;
  (e) read_first == 0 or adapter_first == 0;
  (f) the operations realise the score (gap_extend = gap_open in the linear mode);
  (g) the digest recomputed from the gapped rows H^a V^b P H^c V^d by alignment.cpp's rule is the record itself.
"""
INT_MIN = -2147483648
_CODE = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}
_LET = "ACGTN"


def dna5(ch):
    return _CODE.get(ch, 4)


def oracle_record(r):
    """The oracle's result as the library's 8-int record (the two identities share one match count there)."""
    if r.failed:
        return [-1, 0, -1, 0, INT_MIN, 0, 0, 0]
    assert r.aligned_matches == r.full_matches
    return [r.read_start, r.read_end, r.adapter_start, r.adapter_end, r.score, r.aligned_matches, r.aligned_len, r.full_len]


def digest_of_rows(r0, r1):
    """alignment.cpp:6-111 over two gapped rows -> (read_start, read_end, adapter_start, adapter_end, aligned matches,
    aligned length, full matches, full length)."""
    L = len(r0)
    first = lambda r: next(i for i in range(L) if r[i] != "-")
    last = lambda r: next(i for i in range(L - 1, -1, -1) if r[i] != "-")
    # the first / last column by which BOTH rows have shown a base
    start, end = max(first(r0), first(r1)), min(last(r0), last(r1))
    a_s, a_e = first(r1), last(r1)
    am = sum(1 for i in range(start, end + 1) if r0[i] == r1[i])
    fm = sum(1 for i in range(a_s, a_e + 1) if r0[i] == r1[i])
    rb = lambda k: sum(1 for c in r0[:k] if c != "-")
    ab = lambda k: sum(1 for c in r1[:k] if c != "-")
    return rb(start), rb(end), ab(start), ab(end), am, end - start + 1, fm, a_e - a_s + 1


def replay(read, adapter, head, opstring):
    """-> (end row, end column, counts of = X I D, gapped read row, gapped adapter row over the path); asserts (b)."""
    n, m = len(read), len(adapter)
    assert len(opstring) == int(head[0])
    j, i = int(head[1]), int(head[2])
    cnt = {"=": 0, "X": 0, "I": 0, "D": 0}
    r0, r1 = [], []
    for op in opstring:
        cnt[op] += 1
        if op in "=X":
            assert i < m and j < n, "left the rectangle"
            assert (dna5(read[j]) == dna5(adapter[i])) == (op == "="), "= / X against the bases"
            r0.append(_LET[dna5(read[j])]); r1.append(_LET[dna5(adapter[i])])
            i += 1; j += 1
        elif op == "I":
            assert j < n, "left the rectangle"
            r0.append(_LET[dna5(read[j])]); r1.append("-")
            j += 1
        else:
            assert i < m, "left the rectangle"
            r0.append("-"); r1.append(_LET[dna5(adapter[i])])
            i += 1
    return i, j, cnt, "".join(r0), "".join(r1)


def check_path(read, adapter, scores, rec, head, opstring, want):
    """`want`: the oracle's align_raw result for the pair.  rec / head: sequences of ints."""
    n, m = len(read), len(adapter)
    rec, head = [int(x) for x in rec], [int(x) for x in head]
    if n == 0 or m == 0:
        assert rec == [-1, 0, -1, 0, INT_MIN, 0, 0, 0] and head == [0, 0, 0, 0] and opstring == ""
        return
    L, a, b, opens = head
    i, j, cnt, p0, p1 = replay(read, adapter, head, opstring)
    assert i == m or j == n, "(c) the path does not end in the last row or column"
    assert (i, j) == (want.end_i, want.end_j), "(c) end cell"
    assert a + b + L + (n - want.end_j) + (m - want.end_i) == want.path_len, "(d)"
    assert a == 0 or b == 0, "(e)"
    match, mismatch, gap_open, gap_extend = scores
    if gap_open == gap_extend:
        gap_extend = gap_open
    gaps = cnt["I"] + cnt["D"]
    assert 0 <= opens <= gaps
    assert match * cnt["="] + mismatch * cnt["X"] + opens * gap_open + (gaps - opens) * gap_extend == rec[4], "(f) score"
    code = lambda s: "".join(_LET[dna5(c)] for c in s)
    r0 = code(read[:a]) + "-" * b + p0 + code(read[j:]) + "-" * (m - i)
    r1 = "-" * a + code(adapter[:b]) + p1 + "-" * (n - j) + code(adapter[i:])
    rs, re_, as_, ae, am, al, fm, fl = digest_of_rows(r0, r1)
    assert [rs, re_, as_, ae, rec[4], am, al, fl] == rec and fm == am, "(g) digest of the gapped rows"


def digest_from_path(read, adapter, read_first, adapter_first, opstring):
    """What alignment.cpp derives from the two gapped rows a path stands for -> (read_start, read_end, adapter_start,
    adapter_end, aligned matches, aligned length, full matches, full length); asserts (b) on the way."""
    i, j, _, p0, p1 = replay(read, adapter, (len(opstring), read_first, adapter_first, 0), opstring)
    code = lambda s: "".join(_LET[dna5(c)] for c in s)
    r0 = code(read[:read_first]) + "-" * adapter_first + p0 + code(read[j:]) + "-" * (len(adapter) - i)
    r1 = "-" * read_first + code(adapter[:adapter_first]) + p1 + "-" * (len(read) - j) + code(adapter[i:])
    return digest_of_rows(r0, r1)
