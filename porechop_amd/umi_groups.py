"""UMI groups: which reads come from one molecule, by the edit distance of their UMIs.

  read_keys        RunResult.umis -> one key per read: the UMI of a side, or START+END
  unique_keys      the distinct keys (the nodes) with their read counts; which of them can be linked
  pack             keys -> the two bit planes and the lengths Aligner.umi_neighbours / pc_umi_neighbours take
  neighbours_host  pc_umi_neighbours' contract in numpy: every pair of keys within max_dist edits
  neighbours       the same pairs from the GPU, the keys handed in in kernel_order (by length, then composition)
  group            the nodes and their pairs -> a group id and a representative per node ("directional" or "cluster")
  assign           all of it for a run: the per-read groups and the rows of the groups TSV
  mirror_key       START+END as a read of the molecule's other strand shows it: rc(END)+rc(START)
  canonical        the smaller of a key and its mirror, and whether the mirror was taken: with strands=True the nodes are the
                   canonical keys, a pair also says whether it joins the two keys as they stand or mirrored (flip), and every
                   read gets a strand relative to its group's founder

Plain Python and numpy like discover.cluster_inserts: it loads neither torch nor the library; the all-against-all pass runs on
the GPU when the aligner handed in has umi_neighbours, here otherwise."""
from collections import deque

import numpy as np

BY = ("start", "end", "both")
METHODS = ("directional", "cluster")
MAX_KEY = 64
GROUP_COLUMNS = ["name", "group", "key", "reads_of_key", "group_reads", "group_keys", "representative"]
STRAND_COLUMN = "strand"
_COMPLEMENT = str.maketrans("ACGT", "TGCA")

_CODE = np.full(256, 255, dtype=np.uint8)
for _c, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _l in _letters:
        _CODE[ord(_l)] = _c


def _side_key(umi):
    return None if umi is None else umi[4].upper().replace("U", "T")


def read_keys(umis, by):
    """umis: RunResult.umis -- per read (start, end), each None or (set name, first, length, covered, bases).  by: "start",
    "end" or "both".  -> per read its key or None: the UMI of that side, upper-cased with U -> T; for "both" the start UMI and
    the end UMI as START+END (a read lacking either has no key; the distance is over the concatenation)."""
    if by not in BY:
        raise ValueError("by must be one of %s" % (BY,))
    out = []
    for start, end in umis:
        s, e = _side_key(start), _side_key(end)
        if by == "start":
            out.append(s)
        elif by == "end":
            out.append(e)
        else:
            out.append(None if s is None or e is None else s + "+" + e)
    return out


def bases_of(key):
    """The bases the distance runs over: the key without the '+' of START+END."""
    return key.replace("+", "")


def linkable(key):
    """Can the key have edges?  Not when it is empty, longer than 64 bases or holds a letter outside A C G T."""
    b = bases_of(key)
    return 0 < len(b) <= MAX_KEY and not (set(b) - set("ACGT"))


def mirror_key(key):
    """The key START+END ("both" keys only) as a read of the molecule's other strand shows it: rc(END)+rc(START), on upper-cased
    A C G T.  Its bases are the reverse complement of the key's bases (pcud::mirror of the packed key).  A key holding a letter
    outside A C G T is returned as it is."""
    if "+" not in key:
        raise ValueError("mirror_key is defined for START+END keys only")
    start, end = key.upper().split("+", 1)
    if set(start + end) - set("ACGT"):
        return key
    return end.translate(_COMPLEMENT)[::-1] + "+" + start.translate(_COMPLEMENT)[::-1]


def canonical(key):
    """-> (key', s): key' is the one of key and mirror_key(key) whose bases_of is lexicographically smaller, s = 1 iff the mirror
    was taken.  A tie (a self-mirror key such as AC+GT) and a key holding a letter outside A C G T give (key, 0)."""
    m = mirror_key(key)
    if m is not key and bases_of(m) < bases_of(key.upper()):
        return m, 1
    return key, 0


def unique_keys(read_key):
    """Per-read keys (None: no key) -> (keys, counts, node of each read or -1): the distinct keys in order of first
    appearance and how many reads hold each."""
    index, keys, counts, node = {}, [], [], []
    for k in read_key:
        if k is None:
            node.append(-1)
            continue
        at = index.get(k)
        if at is None:
            at = index[k] = len(keys)
            keys.append(k)
            counts.append(0)
        counts[at] += 1
        node.append(at)
    return keys, counts, node


def pack(keys):
    """Linkable keys -> (planes uint64[n, 2], lens int32[n]): base t of a key has code c (A C G T = 0 1 2 3), bit t of plane 0
    is c & 1, bit t of plane 1 is c >> 1; the bits at and above the length are 0."""
    n = len(keys)
    seqs = [bases_of(k).encode("ascii") for k in keys]
    lens = np.array([len(s) for s in seqs], dtype=np.int32).reshape(n)
    if n == 0:
        return np.zeros((0, 2), dtype=np.uint64), lens
    if lens.max() > MAX_KEY:
        raise ValueError("a key above %d bases cannot be packed" % MAX_KEY)
    codes = _CODE[np.frombuffer(b"".join(s.ljust(MAX_KEY, b"A") for s in seqs), dtype=np.uint8).reshape(n, MAX_KEY)]
    inside = np.arange(MAX_KEY)[None, :] < lens[:, None]
    if (codes[inside] > 3).any():
        raise ValueError("a key with a letter outside A C G T cannot be packed")
    shifts = np.arange(MAX_KEY, dtype=np.uint64)[None, :]
    planes = np.empty((n, 2), dtype=np.uint64)
    for p in (0, 1):
        bit = (((codes >> p) & 1) * inside).astype(np.uint64)
        planes[:, p] = (bit << shifts).sum(axis=1, dtype=np.uint64)
    return planes, lens


def _len_mask(lens):
    lens = np.asarray(lens).astype(np.uint64)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    return np.where(lens >= np.uint64(64), ones, (np.uint64(1) << np.minimum(lens, np.uint64(63))) - np.uint64(1))


def mirror_planes(planes, lens):
    """pcud::mirror in numpy: the planes of every key's reverse complement (base t = 3 - base(len - 1 - t); bits at and above
    the length 0; a length outside 0..64 gives the empty key)."""
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(-1, 2)
    n = planes.shape[0]
    lens = np.asarray(lens, dtype=np.int64).reshape(n)
    lens = np.where((lens >= 0) & (lens <= MAX_KEY), lens, 0)
    bits = np.unpackbits(planes.view(np.uint8).reshape(n, 2, 8), axis=2, bitorder="little")       # [n, 2, 64]
    t = np.arange(MAX_KEY, dtype=np.int64)[None, :]
    src = np.clip(lens[:, None] - 1 - t, 0, MAX_KEY - 1)
    inside = (t < lens[:, None])[:, None, :]
    out = (np.take_along_axis(bits, np.broadcast_to(src[:, None, :], bits.shape), axis=2) ^ 1) & inside
    return np.packbits(out.astype(np.uint8), axis=2, bitorder="little").reshape(n, 16).view(np.uint64).reshape(n, 2)


def neighbours_host(planes, lens, max_dist, strands=False):
    """pc_umi_neighbours in numpy: every pair i < j of the keys whose unit-cost edit distance is <= max_dist -> int32[m, 3]
    rows (i, j, distance), sorted by (i, j).  Plane bits at and above a key's length are ignored; a key whose length is outside
    0..64 has no pairs.  Myers' bit vectors (csrc/pc_umi_dist.h) over uint64, one text key i against every pattern key j > i
    at once; no pair is settled by a bound.  This is the route of aligners without umi_neighbours, and the tests' model.
    strands=True is pc_umi_neighbours_stranded: -> int32[m, 4] rows (i, j, d, flip), d = min(d_same, d_mirror) with d_mirror the
    distance of key i and the mirror of key j (= that of the mirror of key i and key j: the text is mirrored here), flip = 1 iff
    d_mirror < d_same; a row is present iff d <= max_dist."""
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(-1, 2)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    n = lens.shape[0]
    assert planes.shape[0] == n and 0 <= max_dist
    valid = (lens >= 0) & (lens <= MAX_KEY)
    safe = np.where(valid, lens, 0)
    mask = _len_mask(safe)
    p0, p1 = planes[:, 0] & mask, planes[:, 1] & mask
    eq = [~p1 & ~p0 & mask, ~p1 & p0 & mask, p1 & ~p0 & mask, p1 & p0 & mask]
    top = np.maximum(safe - 1, 0).astype(np.uint64)
    one = np.uint64(1)
    mirrored = mirror_planes(planes, safe) if strands else None

    def distances(a0, a1, li, js):
        """the text (planes a0, a1 as ints, li bases) against the pattern keys js"""
        lj = safe[js]
        pv, mv = mask[js].copy(), np.zeros(js.size, dtype=np.uint64)
        score = lj.copy()
        e = [m[js] for m in eq]
        t_top = top[js]
        for t in range(li):
            m = e[((a0 >> t) & 1) | (((a1 >> t) & 1) << 1)]
            xv = m | mv
            xh = (((m & pv) + pv) ^ pv) | m
            ph = mv | ~(xh | pv)
            mh = pv & xh
            score += ((ph >> t_top) & one).astype(np.int64) - ((mh >> t_top) & one).astype(np.int64)
            ph = (ph << one) | one
            mh = mh << one
            pv = mh | ~(xv | ph)
            mv = ph & xv
        return np.where(lj == 0, li, score)

    out = []
    for i in np.nonzero(valid)[0].tolist():
        js = i + 1 + np.nonzero(valid[i + 1:])[0]
        if js.size == 0:
            continue
        li = int(safe[i])
        score = distances(int(p0[i]), int(p1[i]), li, js)
        cols = [None, None, score]
        if strands:
            other = distances(int(mirrored[i, 0]), int(mirrored[i, 1]), li, js)
            cols = [None, None, np.minimum(score, other), (other < score).astype(np.int64)]
        hit = np.nonzero(cols[2] <= max_dist)[0]
        if hit.size:
            out.append(np.stack([np.full(hit.size, i, dtype=np.int64), js[hit]] + [c[hit] for c in cols[2:]], axis=1))
    if not out:
        return np.zeros((0, 4 if strands else 3), dtype=np.int32)
    return np.concatenate(out).astype(np.int32)


def composition(planes, lens):
    """The base counts of packed keys -> int64[n, 4] (A C G T)."""
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(-1, 2)
    n = planes.shape[0]
    bits = np.unpackbits(planes.view(np.uint8).reshape(n, 2, 8), axis=2, bitorder="little")       # [n, 2, 64]
    code = bits[:, 0, :] + 2 * bits[:, 1, :]
    inside = np.arange(MAX_KEY)[None, :] < np.asarray(lens).reshape(n, 1)
    return np.stack([((code == c) & inside).sum(axis=1) for c in range(4)], axis=1).astype(np.int64)


def kernel_order(planes, lens):
    """The order in which the keys go to the kernel: by length, then by composition (counts of A, C, G).  The pairs found do
    not depend on it; the time does -- a wave skips a key's DP only when ALL of its 64 lanes are settled by the lower bound,
    which keys of like composition in one wave make likely, and tiles far apart in length are skipped whole."""
    comp = composition(planes, lens)
    return np.lexsort((comp[:, 2], comp[:, 1], comp[:, 0], np.asarray(lens)))


def neighbours(planes, lens, max_dist, aligner=None, device=None, strands=False):
    """The pairs within max_dist on the GPU (`device`) when the aligner has umi_neighbours, on the host otherwise -> int32[m, 3]
    numpy, sorted by (i, j); with strands=True int32[m, 4] rows (i, j, d, flip) as neighbours_host gives them.  On the GPU the
    keys go in in kernel_order (d_mirror is symmetric in the two keys, so a pair handed back as (j, i) keeps its flip)."""
    if aligner is None or not hasattr(aligner, "umi_neighbours") or len(lens) < 2:
        return neighbours_host(planes, lens, max_dist, strands) if strands else neighbours_host(planes, lens, max_dist)
    import torch
    order = kernel_order(planes, lens)
    dev = "cuda" if device is None else device
    pl = torch.from_numpy(np.ascontiguousarray(planes[order]).view(np.int64)).to(dev)
    ln = torch.from_numpy(np.ascontiguousarray(lens[order], dtype=np.int32)).to(dev)
    got = (aligner.umi_neighbours(pl, ln, int(max_dist), strands=True) if strands else aligner.umi_neighbours(pl, ln, int(max_dist)))
    got = got.cpu().numpy().astype(np.int64)
    if got.shape[0] == 0:
        return np.zeros((0, 4 if strands else 3), dtype=np.int32)
    a, b = order[got[:, 0]], order[got[:, 1]]
    pairs = np.stack([np.minimum(a, b), np.maximum(a, b)] + [got[:, c] for c in range(2, got.shape[1])], axis=1)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.int32)


def group(keys, counts, pairs, method="directional", strands=False):
    """Nodes (keys with their read counts) and their pairs (rows (a, b, ...) of node indices) -> (group id per node, from 1;
    representative key per node: the key that founded its group).
    Nodes are ordered by count descending, then key ascending.
      "directional"  in that order a node not yet in a group founds the next group and takes every ungrouped node reachable
                     from it over edges a -> b: {a, b} is a pair and count(a) >= 2 * count(b) - 1
      "cluster"      connected components over the pairs, numbered by their first node in the same order
    strands=True: the pairs are rows (a, b, d, flip) and a third list comes back, the orientation of every node relative to its
    group's founder: the founder has 0, a node b taken from a has o(a) ^ flip(a, b) -- the walk is the same, so which edge takes
    b is fixed by it."""
    if method not in METHODS:
        raise ValueError("method must be one of %s" % (METHODS,))
    n = len(keys)
    assert len(counts) == n
    adj = [[] for _ in range(n)]
    pairs = np.asarray(pairs)
    for row in (pairs.reshape(-1, pairs.shape[-1]).tolist() if pairs.size else []):
        a, b = int(row[0]), int(row[1])
        flip = int(row[3]) if strands else 0
        adj[a].append((b, flip))
        adj[b].append((a, flip))
    order = sorted(range(n), key=lambda k: (-counts[k], keys[k]))
    gid = [0] * n
    rep = [None] * n
    orient = [0] * n
    groups = 0
    for founder in order:
        if gid[founder]:
            continue
        groups += 1
        gid[founder], rep[founder] = groups, keys[founder]
        todo = deque([founder])
        while todo:
            a = todo.popleft()
            for b, flip in adj[a]:
                if gid[b] == 0 and (method == "cluster" or counts[a] >= 2 * counts[b] - 1):
                    gid[b], rep[b], orient[b] = groups, keys[founder], orient[a] ^ flip
                    todo.append(b)
    return (gid, rep, orient) if strands else (gid, rep)


def groups_header(strands=False):
    return "#" + "\t".join(GROUP_COLUMNS + ([STRAND_COLUMN] if strands else [])) + "\n"


def assign(umis, names, by, max_dist=2, method="directional", max_keys=1 << 20, aligner=None, device=None, strands=False):
    """The groups of a run: umis as RunResult.umis, names the reads' names.  -> (per read None or (group, representative), the
    rows of the groups TSV: one per read with a key, in input order).  A key that cannot be linked (empty, above 64 bases, a
    letter outside A C G T) is a node without edges.  More linkable distinct keys than max_keys raise OverflowError.
    strands=True (by "both" only) groups across both strands of a molecule: the nodes are the distinct CANONICAL keys, their
    counts summed over both orientations (reads_of_key is the node's count); the pairs carry a flip; a read's strand is
    (its key was mirrored to become canonical) ^ (its node's orientation), 0 being the orientation of the founder's canonical
    key.  -> per read None or (group, representative, strand), the representative the founder's canonical key; the rows keep the
    key as read and gain an eighth column: + for strand 0, - for 1."""
    read_key = read_keys(umis, by)
    read_strand = None
    if strands:
        if by != "both":
            raise ValueError("strands needs by == 'both'")
        both = [None if k is None else canonical(k) for k in read_key]
        read_strand = [0 if c is None else c[1] for c in both]
        keys, counts, node = unique_keys([None if c is None else c[0] for c in both])
    else:
        keys, counts, node = unique_keys(read_key)
    link = [k for k in range(len(keys)) if linkable(keys[k])]
    if len(link) > max_keys:
        raise OverflowError(len(link))
    planes, lens = pack([keys[k] for k in link])
    width = 4 if strands else 3
    pairs = neighbours(planes, lens, max_dist, aligner, device, strands=True) if strands else neighbours(planes, lens, max_dist, aligner, device)
    link = np.array(link, dtype=np.int64)
    pairs = (np.stack([link[pairs[:, 0]], link[pairs[:, 1]]] + [pairs[:, c] for c in range(2, width)], axis=1) if pairs.shape[0]
             else np.zeros((0, width), dtype=np.int64))
    if strands:
        gid, rep, orient = group(keys, counts, pairs, method, strands=True)
    else:
        gid, rep = group(keys, counts, pairs, method)
    group_reads, group_keys = {}, {}
    for k in range(len(keys)):
        group_reads[gid[k]] = group_reads.get(gid[k], 0) + counts[k]
        group_keys[gid[k]] = group_keys.get(gid[k], 0) + 1
    per_read, rows = [], []
    for r, k in enumerate(node):
        if k < 0:
            per_read.append(None)
            continue
        row = "%s\t%d\t%s\t%d\t%d\t%d\t%s" % (names[r], gid[k], read_key[r], counts[k], group_reads[gid[k]], group_keys[gid[k]], rep[k])
        if strands:
            strand = read_strand[r] ^ orient[k]
            per_read.append((gid[k], rep[k], strand))
            row += "\t" + "+-"[strand]
        else:
            per_read.append((gid[k], rep[k]))
        rows.append(row + "\n")
    return per_read, "".join(rows)
