"""UMI consensus: one consensus sequence per group of reads (the rule: csrc/pc_consensus.h).

Plain Python and numpy; torch is loaded only on the GPU route (an aligner with consensus_round).  round_host is the whole rule
in numpy -- the route for aligners without consensus_round, and the model the GPU tests compare the kernels with.

A pile-up consensus: every member of a group is aligned to the group's template (a banded global edit distance), the
alignments vote per template column and per insertion slot, the votes are called, and the call is the next round's template.
Not a partial-order or neural polisher.

With a quality table (quality_table(), or any 256 Phred values) every emitted base also gets a quality: the table's entry for
the base's vote margin -- its votes less those of the strongest alternative (call()); fastq_text writes them."""
from collections import namedtuple

import numpy as np

INS_SLOTS = 4
MAX_BAND = 127               # pcc::MAX_BAND: 2 band + 1 cells, at most four to a lane
MAX_LEN_LIMIT = 1 << 24      # pcc::MAX_LEN_LIMIT
INF = 0x3FFFFFFF
ST_ACCEPTED, ST_REJECTED, ST_INVALID = 0, 1, 2
OP_DIAG, OP_DEL, OP_INS = 0, 1, 2
DEFAULTS = dict(min_reads=3, max_reads=256, band=64, rounds=2, max_err_pct=30, max_len=65535)
REPORT_COLUMNS = ("group", "representative", "members", "used", "rejected", "skipped", "rounds", "length", "status")
QUALITY_COLUMNS = ("expected_errors", "low_qual")      # behind status (and minus) when the results carry qualities
QUAL_ENTRIES = 256           # a quality table: one Phred value (0 .. MAX_QUAL) per vote margin 0 .. 255
MAX_QUAL = 93                # Phred + 33 stays printable
LOW_QUAL = 10                # the report's low_qual column counts the bases below this
# the status column: a group is "called" or says why it has no sequence
CALLED, FEW_READS, TOO_LONG, EMPTY, OVER_BUDGET = "called", "few_reads", "too_long", "empty", "over_budget"

_CODE = np.full(256, 4, dtype=np.uint8)
for _c, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _l in _letters:
        _CODE[ord(_l)] = _c
_LETTER = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP_CODE = np.array([3, 2, 1, 0, 4], dtype=np.uint8)        # pcc::comp_code
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")

# One round over several groups.  cons: the consensus bytes of all groups back to back (uint8), lens int32[groups], status and
# distance int32[members], voters int32[groups], votes None or a list of uint32 arrays (21 la + 16 counters per group), qual None
# or one Phred value per byte of cons (uint8, the same layout): a round that was given a quality table.
Round = namedtuple("Round", "cons lens status distance voters votes qual", defaults=(None,))


class OverBudget(RuntimeError):
    """One group alone needs more scratch than PC_CONSENSUS_SCRATCH_MB allows: args[0] is its index in the call."""


def codes(seq):
    """bytes / uint8 array -> base codes (A C G T = 0..3, U as T, either case, anything else 4)."""
    return _CODE[np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)]


def reverse_complement_codes(b):
    """Codes of a member -> the codes it shows when read as strand 1: base j is the complement of base lb - 1 - j (0 <-> 3,
    1 <-> 2, 4 stays 4)."""
    return _COMP_CODE[np.asarray(b, dtype=np.uint8)[::-1]]


def reverse_complement(seq):
    """A consensus (bytes over A C G T) in the other orientation."""
    return seq.translate(_COMPLEMENT)[::-1]


def votes_per_group(la):
    return 21 * la + 4 * INS_SLOTS


def cons_capacity(la):
    return 5 * la + INS_SLOTS


def check_options(min_reads, max_reads, band, rounds, max_err_pct, max_len):
    """-> None, or (the option's name, what is wrong with it)."""
    if int(min_reads) < 2:
        return "min_reads", "must be at least 2: a consensus needs a template and a member aligned to it"
    if int(max_reads) < int(min_reads):
        return "max_reads", "must be at least min_reads"
    if not 1 <= int(band) <= MAX_BAND:
        return "band", "must lie in 1..%d" % MAX_BAND
    if int(rounds) < 1:
        return "rounds", "must be at least 1"
    if not 0 <= int(max_err_pct) <= 100:
        return "max_err_pct", "must lie in 0..100"
    if not 1 <= int(max_len) <= MAX_LEN_LIMIT:
        return "max_len", "must lie in 1..%d" % MAX_LEN_LIMIT
    return None


# ---- the rule in numpy --------------------------------------------------------------------------------------------------------
def align(a, b, band):
    """Codes a (template, la >= 1) and b (member) -> (banded distance, INF when no path stays inside the band; the trace: uint8
    [la + 1, 2 band + 1] of OP_*, row i's cell k being column floor(i lb / la) - band + k).  A row is swept at once: the cell to
    the left enters as a min-plus prefix, D[k] = k + min over k' <= k of (t[k'] - k')."""
    la, lb = len(a), len(b)
    assert la >= 1 and band >= 1
    W = 2 * band + 1
    ks = np.arange(W, dtype=np.int64)
    bpad = np.concatenate([np.array([4], dtype=np.uint8), np.asarray(b, dtype=np.uint8)])      # b[j - 1] at j
    lo = -band
    j = lo + ks
    row = np.where((j >= 0) & (j <= lb), j, INF).astype(np.int64)
    ops = np.full((la + 1, W), OP_INS, dtype=np.uint8)
    for i in range(1, la + 1):
        lo_new = i * lb // la - band
        sh = lo_new - lo
        j = lo_new + ks
        valid = (j >= 0) & (j <= lb)
        up = np.full(W, INF, dtype=np.int64)
        if sh < W:
            up[:W - sh] = row[sh:]
        dg = np.full(W, INF, dtype=np.int64)
        if sh == 0:
            dg[1:] = row[:-1]
        elif sh - 1 < W:
            dg[:W - (sh - 1)] = row[sh - 1:]
        ca = int(a[i - 1])
        cb = bpad[np.clip(j, 0, lb)]
        cost = np.where((cb == ca) & (ca < 4), 0, 1)
        dv = np.where(valid & (j >= 1), dg + cost, INF)
        uv = up + 1
        t = np.where(valid, np.minimum(dv, uv), INF)
        v = np.minimum.accumulate(t - ks) + ks
        v = np.where(valid & (v < INF), v, INF)
        ops[i] = np.where(valid, np.where(dv == v, OP_DIAG, np.where(uv == v, OP_DEL, OP_INS)), OP_INS)
        row, lo = v, lo_new
    return int(row[band]), ops


def rejected(d, la, lb, max_err_pct):
    return d * 100 > max_err_pct * max(la, lb)


def walk(b, la, band, ops, votes):
    """The path from (la, lb) back to (0, 0) in csrc/pc_consensus.h's order -- diagonal, else the template column, else the
    member base -- adding the member's votes to `votes` (one group's counters)."""
    lb = len(b)
    i, j = la, lb
    W = 2 * band + 1

    def op_at(i, j):
        k = j - (i * lb // la - band)
        assert 0 <= k < W, "the walk left its band"
        return int(ops[i, k])

    while i > 0 or j > 0:
        op = OP_INS if i == 0 else (OP_DEL if j == 0 else op_at(i, j))
        if op == OP_DIAG:
            c = int(b[j - 1])
            if c < 4:
                votes[5 * (i - 1) + c] += 1
            i, j = i - 1, j - 1
        elif op == OP_DEL:
            votes[5 * (i - 1) + 4] += 1
            i -= 1
        else:
            run = 1
            while j - run > 0 and (i == 0 or op_at(i, j - run) == OP_INS):
                run += 1
            for s in range(min(run, INS_SLOTS)):
                c = int(b[j - run + s])
                if c < 4:
                    votes[5 * la + (i * INS_SLOTS + s) * 4 + c] += 1
            j -= run


def quality_table(vote_err_pct=10, max_qual=60):
    """The default quality table: uint8[256], entry m the Phred value of a base whose vote margin is m (255: that or more).
    Under independent votes, each wrong with probability e = vote_err_pct / 100 and then on each of the four alternatives
    alike, the likelihood ratio of the leader against one alternative is r^m with r = 4 (1 - e) / e; with all four
    alternatives as strong as the runner-up P(wrong) <= 4 / (4 + r^m), so entry m = min(max_qual, round(10 log10(1 + r^m /
    4))), computed in logs.  vote_err_pct in 1 .. 50 and max_qual in 1 .. 93, else ValueError."""
    if isinstance(vote_err_pct, bool) or int(vote_err_pct) != vote_err_pct or not 1 <= int(vote_err_pct) <= 50:
        raise ValueError("vote_err_pct must be a whole number in 1..50")
    if isinstance(max_qual, bool) or int(max_qual) != max_qual or not 1 <= int(max_qual) <= MAX_QUAL:
        raise ValueError("max_qual must be a whole number in 1..%d" % MAX_QUAL)
    e = int(vote_err_pct) / 100.0
    x = np.arange(QUAL_ENTRIES, dtype=np.float64) * np.log(4.0 * (1.0 - e) / e) - np.log(4.0)       # ln(r^m / 4)
    phred = 10.0 * np.logaddexp(0.0, x) / np.log(10.0)
    return np.minimum(np.floor(phred + 0.5), int(max_qual)).astype(np.uint8)


def check_quality_table(qual_table):
    """-> the table as uint8[256]; ValueError when it is not 256 values in 0 .. 93."""
    t = np.asarray(qual_table)
    if t.shape != (QUAL_ENTRIES,) or t.dtype.kind not in "ui" or int(t.min()) < 0 or int(t.max()) > MAX_QUAL:
        raise ValueError("a quality table is %d whole numbers in 0..%d" % (QUAL_ENTRIES, MAX_QUAL))
    return np.ascontiguousarray(t, dtype=np.uint8)


def call(votes, a, voters, qual_table=None, tmpl_counts=1):
    """One group's counters, the template's codes and the voters -> the consensus bytes.  The template's own vote is added to
    `votes` first.  Column: the leader, nothing when deletion leads; ties to the template's base when it leads, else the
    smallest of A < C < G < T < deletion.  Slot: emitted iff twice its sum exceeds voters; its leader, ties to the smallest.
    With qual_table (uint8[256]) -> (the bytes, one Phred value per byte: uint8): qual_table[min(margin, 255)] of the emitted
    base's vote margin (pcc::column_margin, pcc::slot_margin).  Column, called base b: e = the five counters, less the
    template's own vote when tmpl_counts is 0 (an earlier consensus decides ties but is no evidence); margin = max(0, e[b] -
    max over k != b of e[k]), deletion among the k.  Slot, emitted base b: absent = voters - the slot's sum; margin = max(0,
    cnt[b] - max(absent, max over k != b of cnt[k]))."""
    la = len(a)
    a = np.asarray(a, dtype=np.int64)
    cols = votes[:5 * la].reshape(la, 5)
    own = np.nonzero(a < 4)[0]
    cols[own, a[own]] += 1
    top = cols.max(axis=1)
    pick = cols.argmax(axis=1)                                  # the first leader: the smallest
    own_leads = np.zeros(la, dtype=bool)
    own_leads[own] = cols[own, a[own]] == top[own]
    pick = np.where(own_leads, a, pick)
    slots = votes[5 * la:].reshape(la + 1, INS_SLOTS, 4)
    emit = 2 * slots.sum(axis=2, dtype=np.int64) > voters
    out = np.zeros((la + 1, INS_SLOTS + 1), dtype=np.uint8)
    keep = np.zeros((la + 1, INS_SLOTS + 1), dtype=bool)
    out[:, :INS_SLOTS] = _LETTER[slots.argmax(axis=2)]
    keep[:, :INS_SLOTS] = emit
    out[:la, INS_SLOTS] = _LETTER[np.minimum(pick, 3)]
    keep[:la, INS_SLOTS] = pick < 4
    if qual_table is None:
        return out[keep].tobytes()
    e = cols.astype(np.int64)
    if not int(tmpl_counts):
        e[own, a[own]] -= 1
    rows = np.arange(la)
    lead = e[rows, np.minimum(pick, 4)]
    rest = e.copy()
    rest[rows, np.minimum(pick, 4)] = -1
    margin = np.zeros((la + 1, INS_SLOTS + 1), dtype=np.int64)
    margin[:la, INS_SLOTS] = lead - rest.max(axis=1)
    cnt = slots.astype(np.int64)
    best = cnt.argmax(axis=2)
    top_slot = np.take_along_axis(cnt, best[:, :, None], axis=2)[:, :, 0]
    others = cnt.copy()
    np.put_along_axis(others, best[:, :, None], -1, axis=2)
    margin[:, :INS_SLOTS] = top_slot - np.maximum(int(voters) - cnt.sum(axis=2), others.max(axis=2))
    qual = np.asarray(qual_table, dtype=np.uint8)[np.clip(margin, 0, QUAL_ENTRIES - 1)]
    return out[keep].tobytes(), qual[keep]


def round_host(tmpls, member_seqs, member_group, band, max_err_pct, max_len=DEFAULTS["max_len"], tmpl_counts=1, return_votes=False,
               member_strand=None, qual_table=None):
    """One round in numpy: tmpls a list of byte strings (one per group), member_seqs a list of byte strings, member_group their
    groups -> Round.  A template or member outside 1 / 0 .. max_len is what the library reports at sync(): here its members are
    ST_INVALID with distance -1, and such a group's consensus is empty.  member_strand: None (all 0) or one 0 / 1 per member --
    a member of strand 1 is read as its reverse complement (pc_consensus_round_stranded); templates are never flipped.
    qual_table: None, or uint8[256] -- Round.qual then holds one Phred value per consensus byte (pc_consensus_round_quality)."""
    G, M = len(tmpls), len(member_seqs)
    if qual_table is not None:
        qual_table = check_quality_table(qual_table)
    if G == 0 or M == 0:                                         # the library's no-op
        return Round(np.zeros(0, dtype=np.uint8), np.zeros(G, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
                     np.zeros(G, dtype=np.int32), [np.zeros(votes_per_group(len(t)), dtype=np.uint32) for t in tmpls] if return_votes else None,
                     None if qual_table is None else np.zeros(0, dtype=np.uint8))
    status = np.zeros(M, dtype=np.int32)
    distance = np.zeros(M, dtype=np.int32)
    voters = np.full(G, int(tmpl_counts), dtype=np.int32)
    a_codes = [codes(t) for t in tmpls]
    fine = [1 <= len(t) <= max_len for t in tmpls]
    votes = [np.zeros(votes_per_group(len(t)) if ok else 0, dtype=np.uint32) for t, ok in zip(tmpls, fine)]
    for m in range(M):
        g = int(member_group[m])
        b = codes(member_seqs[m])
        if member_strand is not None and int(member_strand[m]):
            b = reverse_complement_codes(b)
        if not fine[g] or len(b) > max_len:
            status[m], distance[m] = ST_INVALID, -1
            continue
        la = len(a_codes[g])
        d, ops = align(a_codes[g], b, band)
        distance[m] = d
        if rejected(d, la, len(b), max_err_pct):
            status[m] = ST_REJECTED
            continue
        walk(b, la, band, ops, votes[g])
        voters[g] += 1
    qual = None
    if qual_table is None:
        cons = [call(votes[g], a_codes[g], int(voters[g])) if fine[g] else b"" for g in range(G)]
    else:
        both = [call(votes[g], a_codes[g], int(voters[g]), qual_table, tmpl_counts) if fine[g] else (b"", np.zeros(0, dtype=np.uint8))
                for g in range(G)]
        cons = [c for c, _q in both]
        qual = np.concatenate([q for _c, q in both]).astype(np.uint8)
    return Round(np.frombuffer(b"".join(cons), dtype=np.uint8), np.array([len(c) for c in cons], dtype=np.int32), status, distance, voters,
                 votes if return_votes else None, qual)


# ---- members and templates ----------------------------------------------------------------------------------------------------
def members(umi_groups, lengths, start_trim, end_trim, piece_read, piece_number):
    """Which reads are members of which group.  umi_groups as RunResult.umi_groups (per read None or (group, representative) --
    or (group, representative, strand) of a run over both strands; the strand is not looked at here),
    the trims per read, and the piece plan (per piece its read and its number: 0 for an unsplit read).  A member is a read of a
    group that is written as exactly ONE piece -- not split or discarded -- with at least one base left; its sequence is the
    trimmed read [start_trim, length - end_trim).  -> [(group, representative, [reads in input order])] in group order."""
    whole = np.zeros(len(lengths), dtype=np.int64)
    pr = np.asarray(piece_read, dtype=np.int64)
    np.add.at(whole, pr, 1)
    single = whole == 1
    single[pr[np.asarray(piece_number) != 0]] = False
    by_group = {}
    for r, entry in enumerate(umi_groups):
        if entry is None:
            continue
        g, rep = entry[0], entry[1]
        reads = by_group.setdefault(g, (rep, []))[1]
        if single[r] and int(lengths[r]) - int(end_trim[r]) - int(start_trim[r]) >= 1:
            reads.append(r)
    return [(g, by_group[g][0], by_group[g][1]) for g in sorted(by_group)]


def template(lens):
    """The round-1 template of a group whose members have these lengths, in input order: the lower median by (length, input
    order) -> its index."""
    order = sorted(range(len(lens)), key=lambda k: (int(lens[k]), k))
    return order[(len(order) - 1) // 2]


# ---- the rounds ----------------------------------------------------------------------------------------------------------------
def _round(aligner, arena, dev_arena, device, tmpl_bytes, tmpl_src, seq_off, seq_len, member_reads, member_group, band, max_err_pct,
           max_len, tmpl_counts, member_strand=None, qual_table=None):
    """One round over the open groups on the library when the aligner has consensus_round, in numpy otherwise.  tmpl_src: per
    group the read that is the template (round 1), or None when tmpl_bytes holds earlier consensus sequences.  member_strand:
    None, or per member whether this round reads it as its reverse complement.  qual_table: None, or the quality table."""
    strand_kw = {} if member_strand is None else dict(member_strand=np.asarray(member_strand, dtype=np.uint8))
    if qual_table is not None:
        strand_kw["qual_table"] = qual_table
    if aligner is None or not hasattr(aligner, "consensus_round"):
        return round_host(tmpl_bytes, [arena[seq_off[r]:seq_off[r] + seq_len[r]].tobytes() for r in member_reads], member_group, band,
                          max_err_pct, max_len, tmpl_counts, **strand_kw)
    import torch
    tmpl_len = np.array([len(t) for t in tmpl_bytes], dtype=np.int32)
    if tmpl_src is not None:
        tmpl_arena, tmpl_off = dev_arena, np.array([seq_off[r] for r in tmpl_src], dtype=np.int64)
    else:                                                          # the earlier consensus sequences: a small arena of their own
        tmpl_off = np.concatenate([[0], np.cumsum(tmpl_len[:-1], dtype=np.int64)]).astype(np.int64)
        tmpl_arena = torch.from_numpy(np.frombuffer(b"".join(tmpl_bytes) + bytes(64), dtype=np.uint8).copy()).to(device)
    return aligner.consensus_round(dev_arena, tmpl_off, tmpl_len, np.asarray([seq_off[r] for r in member_reads], dtype=np.int64),
                                   np.asarray([seq_len[r] for r in member_reads], dtype=np.int32), np.asarray(member_group, dtype=np.int32),
                                   band, max_err_pct, max_len=max_len, tmpl_counts=tmpl_counts, tmpl_arena=tmpl_arena, **strand_kw)


def call_groups(groups, arena, seq_off, seq_len, min_reads=3, max_reads=256, band=64, rounds=2, max_err_pct=30, max_len=65535,
                aligner=None, dev_arena=None, device=None, read_strand=None, qual_table=None):
    """The consensus of every group.  groups as members() gives them; arena the reads' bytes (numpy uint8), seq_off / seq_len per
    READ the offset and length of its trimmed sequence in it; dev_arena the same arena on the device (for an aligner with
    consensus_round).  -> one dict per group, in group order: group, representative, members, used (accepted in the last
    round, the template read included), rejected, skipped (members beyond max_reads, or above max_len), rounds, length, status,
    sequence (bytes, None unless status is "called").
    read_strand: None, or per READ its strand in its group (0: the orientation of the founder's canonical key, 1: the other
    strand; umi_groups.assign(strands=True)).  Round 1 runs in the orientation of its template read: the device is given
    strand(member) ^ strand(template read), and when the template read is of strand 1 the round's consensus is
    reverse-complemented here, on its way to being the next round's template; from round 2 on the device is given
    strand(member).  Every sequence returned is in the group's strand-0 orientation, and every dict gains `minus`: how many of
    the members that enter the pile-up (the template read included) are read as their reverse complement.
    qual_table: None, or uint8[256] (quality_table()) -- every dict gains `quality`: for a called group one Phred value per base
    of `sequence` (bytes of 0 .. 93, not ASCII), else None.  The qualities travel with the sequence: every round replaces them,
    a round that returns its template ends the group with that round's qualities, and where the round-1 consensus of a
    strand-1 template read is reverse-complemented they are reversed."""
    if qual_table is not None:
        qual_table = check_quality_table(qual_table)
    bad = check_options(min_reads, max_reads, band, rounds, max_err_pct, max_len)
    if bad:
        raise ValueError("%s %s" % bad)
    out, open_ = [], []
    for g, rep, reads in groups:
        taking = [r for r in reads if seq_len[r] >= 1][:max_reads]      # (a read without a base is no member: counted as skipped)
        row = dict(group=g, representative=rep, members=len(reads), used=0, rejected=0, skipped=len(reads) - len(taking), rounds=0, length=0,
                   status=CALLED, sequence=None)
        if qual_table is not None:
            row["quality"] = None
        if read_strand is not None:
            row["minus"] = 0
        out.append(row)
        if len(reads) < min_reads:
            row["status"] = FEW_READS
            continue
        first = taking[template([seq_len[r] for r in taking])]
        if seq_len[first] > max_len:
            row["status"] = TOO_LONG
            continue
        part = [r for r in taking if seq_len[r] <= max_len]          # a member above max_len sits out
        row["skipped"] = len(reads) - len(part)
        if len(part) < 2:                                            # nobody left to align to the template
            row["status"] = FEW_READS
            continue
        row.update(part=part, first=first, tmpl=arena[seq_off[first]:seq_off[first] + seq_len[first]].tobytes())
        if read_strand is not None:
            row["minus"] = sum(int(read_strand[r]) for r in part)
        open_.append(row)
    for rnd in range(1, int(rounds) + 1):
        if not open_:
            break
        while True:
            member_reads, member_group = [], []
            member_strand = None if read_strand is None else []
            for k, row in enumerate(open_):
                for r in row["part"]:
                    if rnd > 1 or r != row["first"]:
                        member_reads.append(r)
                        member_group.append(k)
                        if member_strand is not None:        # round 1 runs in the orientation of its template read
                            member_strand.append(int(read_strand[r]) ^ (int(read_strand[row["first"]]) if rnd == 1 else 0))
            try:
                res = _round(aligner, arena, dev_arena, device, [row["tmpl"] for row in open_],
                             [row["first"] for row in open_] if rnd == 1 else None, seq_off, seq_len, member_reads, member_group, int(band),
                             int(max_err_pct), int(max_len), 1 if rnd == 1 else 0, member_strand, qual_table)
                break
            except OverBudget as e:                                  # that group is refused; the others go on
                open_.pop(int(e.args[0]))["status"] = OVER_BUDGET
                if not open_:
                    res = None
                    break
        if res is None:
            break
        ends = np.cumsum(res.lens, dtype=np.int64)
        still = []
        for k, row in enumerate(open_):
            seq = res.cons[ends[k] - res.lens[k]:ends[k]].tobytes()
            qual = None if qual_table is None else np.asarray(res.qual[ends[k] - res.lens[k]:ends[k]], dtype=np.uint8).tobytes()
            row["rounds"], row["used"] = rnd, int(res.voters[k])
            row["rejected"] = len(row["part"]) - row["used"]
            if not seq or len(seq) > max_len:
                row["status"] = EMPTY if not seq else TOO_LONG
                continue
            unchanged = seq == row["tmpl"]
            if rnd == 1 and read_strand is not None and int(read_strand[row["first"]]):
                seq = reverse_complement(seq)                        # the template read was of strand 1: now the group's orientation
                qual = None if qual is None else qual[::-1]
            row["tmpl"], row["qual"] = seq, qual
            if not unchanged:                                        # a round that returns its template ends the group
                still.append(row)
        open_ = still
    for row in out:
        tmpl = row.pop("tmpl", None)
        row.pop("part", None)
        row.pop("first", None)
        qual = row.pop("qual", None)
        if row["status"] == CALLED:
            row["sequence"], row["length"] = tmpl, len(tmpl)
            if qual_table is not None:
                row["quality"] = qual
    return out


# ---- writers -------------------------------------------------------------------------------------------------------------------
def fasta_text(results):
    """One record per called group, in group order.  Results of a run over both strands (dicts with `minus`) say minus=<members
    read as their reverse complement> after reads=."""
    return "".join(">umi_group_%d key=%s reads=%d%s used=%d rounds=%d length=%d\n%s\n" % (
        r["group"], r["representative"], r["members"], " minus=%d" % r["minus"] if "minus" in r else "", r["used"], r["rounds"], r["length"],
        r["sequence"].decode("ascii"))
        for r in results if r["status"] == CALLED)


def fastq_text(results):
    """One FASTQ record per called group of results that carry `quality`, in group order: fasta_text's header behind '@', the
    sequence, '+', the qualities as Phred + 33."""
    return "".join("@" + fasta_text([r])[1:] + "+\n" + bytes(q + 33 for q in r["quality"]).decode("ascii") + "\n"
                   for r in results if r["status"] == CALLED)


def expected_errors(quality):
    """Phred values (bytes) -> (the sum over the bases of 10^(-q / 10), how many lie below LOW_QUAL); (0.0, 0) for None."""
    if not quality:
        return 0.0, 0
    q = np.frombuffer(quality, dtype=np.uint8)
    return float(np.sum(10.0 ** (-q.astype(np.float64) / 10.0))), int((q < LOW_QUAL).sum())


def report_text(results, minus=None, quality=None):
    """The TSV: a '#' header and one row per group; a column `minus` behind status for the results of a run over both strands
    (minus: None reads that off the results), and behind that QUALITY_COLUMNS for results that carry `quality` (quality: None
    reads that off the results): expected_errors %.3f and low_qual, 0.000 and 0 for a row without a sequence."""
    minus = (bool(results) and all("minus" in r for r in results)) if minus is None else bool(minus)
    quality = (bool(results) and all("quality" in r for r in results)) if quality is None else bool(quality)
    return "#" + "\t".join(REPORT_COLUMNS + (("minus",) if minus else ()) + (QUALITY_COLUMNS if quality else ())) + "\n" + "".join(
        "%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s" % tuple(r[c] for c in REPORT_COLUMNS) + ("\t%d" % r["minus"] if minus else "") +
        ("\t%.3f\t%d" % expected_errors(r.get("quality")) if quality else "") + "\n"
        for r in results)
