"""A model, in plain Python, of the BLOCK logic of the row-skipping score kernel (csrc/pc_jit_source.h, PC_SKIP), held against
the plain recurrence: the one-column path at a window's head and tail, stretches of 4-column fast-path blocks that compute
the rows <= r0 always and the rows below only while a window is open -- opened for W_low columns on entering a stretch and
by a trigger (M(r0, j) >= theta in either half) on any of a block's four columns, re-armed by a second trigger inside it,
expiring, the rows below reset to -infinity when it does -- the rows below kept apart from the upper ones during a stretch
(the kernel's LDS copy) under a renormalisation that shifts every stored value, and the hand-over of their state at both
ends of a stretch.  What is checked is the proposition's outcome (csrc/pc_bounds.h): M^ <= M everywhere, and every
candidate end cell with M >= F exact.  The thresholds are pc_bounds.h's formulas restated; tests/test_row_skip_host.py
holds the header itself."""
import random

NEG = float("-inf")
SCORES = (3, -6, -5, -2)
Y28, Y22 = "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"
A33, A30 = "GCTTGGGTGTTTAACCGTTTTCGCATTTATCGT", "CACAAAGACACCGACAACTTTCTTCAGCAC"


def column(state, base, ad, rows):
    """One column over the adapter rows in `rows` (1-based, top to bottom).  state: M, H, V and Mprev (M of the column before)
    indexed by row; the row above the first one must hold this column's M and V already."""
    match, mismatch, go, ge = SCORES
    M, H, V, Mprev = state["M"], state["H"], state["V"], state["Mprev"]
    for i in rows:
        h = max(H[i] + ge, Mprev[i] + go)
        v = max(V[i - 1] + ge, M[i - 1] + go)
        d = Mprev[i - 1] + (match if base == ad[i - 1] else mismatch)
        M[i], H[i], V[i] = max(d, h, v), h, v


def plain(read, ad):
    m, n = len(ad), len(read)
    out = [[0] * (m + 1)]
    st = {"M": [0] * (m + 1), "H": [NEG] * (m + 1), "V": [NEG] * (m + 1), "Mprev": None}
    for j in range(1, n + 1):
        st["Mprev"] = list(st["M"])
        column(st, read[j - 1], ad, range(1, m + 1))
        out.append(list(st["M"]))
    return out


def end_cells(read, ads, i0s, thetas, w_low, tf, kren, floors, reset=True):
    """Run the model; compare what the kernel compares: tracked last-row cells (columns > tf) and the last column's cells."""
    n = len(read)
    halves, blocks, on_blocks = skipping_tracked(read, ads, i0s, thetas, w_low, tf, kren, reset)
    for h, ad, F in zip(halves, ads, floors):
        full = plain(read, ad)
        m = len(ad)
        for j in range(1, n + 1):
            got = h["last_row"][j]
            assert got <= full[j][m], (j, got, full[j][m])
            if j > tf and full[j][m] >= F:
                assert got == full[j][m], ("last row", j, got, full[j][m])
        if n:
            for i in range(1, m + 1):
                assert h["last_col"][i] <= full[n][i]
                if full[n][i] >= F:
                    assert h["last_col"][i] == full[n][i], ("last column", i)
    return blocks, on_blocks


def skipping_tracked(read, ads, i0s, thetas, w_low, tf, kren, reset=True):
    """The model, with per half the last row's M^ of every column (-infinity where the rows below are off) and the last column."""
    last_rows = [[NEG] * (len(read) + 1) for _ in ads]
    halves, blocks, on_blocks = skipping_with_hook(read, ads, i0s, thetas, w_low, tf, kren, last_rows, reset)
    for q, h in enumerate(halves):
        h["last_row"] = last_rows[q]
        h["last_col"] = list(h["M"])
    return halves, blocks, on_blocks


def skipping_with_hook(read, ads, i0s, thetas, w_low, tf, kren, last_rows, reset=True):
    """The model proper: after every column the last row's value goes to last_rows[half][j].  reset=False leaves the rows below
    as they stand when a window runs out (test_the_model_can_fail)."""
    n = len(read)
    halves = [{"M": [0] * (len(ad) + 1), "H": [NEG] * (len(ad) + 1), "V": [NEG] * (len(ad) + 1), "Mprev": None, "ad": ad, "m": len(ad)}
              for ad in ads]
    blocks = on_blocks = 0
    shift, since = 0, 0
    j0 = 1
    in_stretch, low_until, low_on = False, 0, False
    while j0 <= n:
        if since >= kren:                                 # the renormalisation: every stored value is held minus `shift`, the copy
            shift += 7                                    # of the rows below included (-infinity stays -infinity)
            since = 0
            if in_stretch:
                for h in halves:
                    h["low"] = [(a - 7, b - 7) for a, b in h["low"]]
        fast = j0 > tf and j0 + 3 < n
        if fast and not in_stretch:
            in_stretch, low_until, low_on = True, j0 + 3 + w_low, True
            for h, i0 in zip(halves, i0s):
                h["low"] = [(h["M"][i] - shift, h["H"][i] - shift) for i in range(i0 + 1, h["m"] + 1)]
        if not fast and in_stretch:
            in_stretch = False
            for h, i0 in zip(halves, i0s):
                for k, i in enumerate(range(i0 + 1, h["m"] + 1)):
                    h["M"][i], h["H"][i] = h["low"][k][0] + shift, h["low"][k][1] + shift
        if fast:
            blocks += 1
            upper = [[] for _ in halves]
            trig = False
            for j in range(j0, j0 + 4):
                for q, (h, i0, th) in enumerate(zip(halves, i0s, thetas)):
                    h["Mprev"] = list(h["M"])
                    column(h, read[j - 1], h["ad"], range(1, i0 + 1))
                    upper[q].append((h["Mprev"][i0], h["M"][i0], h["V"][i0]))
                    trig |= h["M"][i0] >= th
            if trig:
                low_until = j0 + 3 + w_low
            if j0 <= low_until:
                low_on = True
                on_blocks += 1
                for q, (h, i0) in enumerate(zip(halves, i0s)):
                    rows = list(range(i0 + 1, h["m"] + 1))
                    Ml = {i: h["low"][k][0] + shift for k, i in enumerate(rows)}
                    Hl = {i: h["low"][k][1] + shift for k, i in enumerate(rows)}
                    for c, j in enumerate(range(j0, j0 + 4)):
                        st = {"M": {i0: upper[q][c][1]}, "H": dict(Hl), "V": {i0: upper[q][c][2]}, "Mprev": dict(Ml)}
                        st["Mprev"][i0] = upper[q][c][0]
                        column(st, read[j - 1], h["ad"], rows)
                        Ml = {i: st["M"][i] for i in rows}
                        Hl = {i: st["H"][i] for i in rows}
                        last_rows[q][j] = Ml[h["m"]]
                    h["low"] = [(Ml[i] - shift, Hl[i] - shift) for i in rows]
            elif low_on:
                for h, i0 in zip(halves, i0s):
                    if reset:
                        h["low"] = [(NEG, NEG)] * (h["m"] - i0)
                low_on = False
        else:
            for j in range(j0, min(j0 + 4, n + 1)):
                for q, h in enumerate(halves):
                    h["Mprev"] = list(h["M"])
                    column(h, read[j - 1], h["ad"], range(1, h["m"] + 1))
                    last_rows[q][j] = h["M"][h["m"]]
        j0 += 4
        since += 4
    if in_stretch:                                        # (a stretch never reaches the last column: the kernel's j0 + 3 < n)
        raise AssertionError("a stretch ran to the end of the window")
    return halves, blocks, on_blocks


def plan(ads, r0, floors):
    """pc_bounds.h row_skip_plan restated: per half theta, and W_low."""
    match, mismatch, go, ge = SCORES
    R = max(len(a) for a in ads)
    g = min(-go, -ge)
    thetas = [F - match * (R - r0) for F in floors]
    assert all(t > 0 for t in thetas)
    w = (R - r0) + max((match * len(a) - F) // g for a, F in zip(ads, floors))
    i0s = [r0 - (R - len(a)) for a in ads]
    return i0s, thetas, w


def mutate(rng, s, k):
    s = list(s)
    for _ in range(k):
        i = rng.randrange(len(s))
        x = rng.random()
        if x < 0.5:
            s[i] = rng.choice("ACGT")
        elif x < 0.75:
            del s[i]
        else:
            s.insert(i, rng.choice("ACGT"))
    return "".join(s)


def make_read(rng, n, ads, copies):
    body = [rng.choice("ACGT") for _ in range(n)]
    for pos, a, k in copies:
        c = mutate(rng, ads[a], k)
        for q, ch in enumerate(c):
            if 0 <= pos + q < n:
                body[pos + q] = ch
    return "".join(body)


CASES = [
    # (adapters, r0, floors, n, tf, kren, copies [(position, adapter, edits)])
    ((Y28, Y22), 20, (58, 46), 400, 0, 1 << 20, [(100, 0, 0), (250, 1, 1)]),                 # trigger, window expiring, a second one later
    ((Y28, Y22), 20, (58, 46), 400, 0, 1 << 20, [(100, 0, 1), (100 + 28 + 8, 0, 0), (180, 1, 0)]),   # re-armed inside W_low
    ((Y28, Y22), 22, (46, 36), 300, 0, 16, [(60, 0, 2), (101, 1, 1), (102 + 40, 0, 0)]),     # a renormalisation inside open windows
    ((A33, A30), 20, (69, 63), 500, 120, 32, [(100, 0, 0), (118, 1, 0), (330, 0, 2), (470, 1, 0)]),  # slow -> fast -> slow, lead-in
    ((A33, A30), 22, (54, 49), 203, 0, 1 << 20, [(-10, 0, 0), (203 - 20, 1, 0)]),            # cut by the start, hanging over the end
    ((Y28, Y28), 20, (58, 58), 120, 0, 24, [(1, 0, 0), (61, 0, 1), (62, 0, 1), (63, 0, 3)]),  # each residue of the block
    ((Y22, Y22), 16, (46, 46), 64, 0, 1 << 20, []),
    ((Y28, Y22), 20, (58, 46), 7, 0, 1 << 20, []),                                          # no fast block at all
]


def test_block_logic_against_the_plain_recurrence():
    rng = random.Random(7)
    saw_on = saw_off = saw_reset = 0
    for ads, r0, floors, n, tf, kren, copies in CASES:
        i0s, thetas, w = plan(ads, r0, floors)
        for rep in range(3):
            read = make_read(rng, n, ads, copies)
            blocks, on = end_cells(read, ads, i0s, thetas, w, tf, kren, floors)
            saw_on += on
            saw_off += blocks - on
            saw_reset += 0 < on < blocks
    assert saw_on > 0 and saw_off > 0 and saw_reset >= 6


def fails(*args, **kw):
    try:
        end_cells(*args, **kw)
    except AssertionError:
        return True
    return False


def test_the_model_can_fail():
    """The four ways to get it wrong that the kernel and pc_bounds.h must not take, each on the smallest input that shows it:
    theta one too high, W_low one block too short, the reset left out when a window runs out, and theta <= 0 accepted."""
    rng = random.Random(11)
    ads = (Y28, Y28)
    # At the floor of 100 % (F = 3 * 28 = 84) an exact copy reaches row r0 = 20 with M = 60 = theta in one column only, and
    # its path needs all of W_low = R - r0 = 8 columns behind it.  The copy starts at a multiple of 4, so that column is a
    # block's last one and the blocks' granularity lends the window nothing.
    floors = (84, 84)
    i0s, thetas, w = plan(ads, 20, floors)
    assert (thetas, w) == ([60, 60], 8)
    for pos in (120, 121, 122, 123):
        read = make_read(rng, 300, ads, [(pos, 0, 0)])
        assert plain(read, Y28)[pos + 28][28] == 84
        end_cells(read, ads, i0s, thetas, w, 0, 1 << 20, floors)
        assert fails(read, ads, i0s, [61, 61], w, 0, 1 << 20, floors), "theta + 1 lost nothing"
        if pos == 120:
            assert fails(read, ads, i0s, thetas, w - 4, 0, 1 << 20, floors), "a window one block shorter lost nothing"
    # A copy, its window running out, and 20 exact rows of a second copy behind it: without the reset the second window
    # starts from what the first one left and the last row comes out ABOVE the true matrix (claim 1).
    floors = (58, 58)
    i0s, thetas, w = plan(ads, 20, floors)
    body = [rng.choice("ACGT") for _ in range(400)]
    body[100:128] = Y28
    body[200:220] = Y28[:20]
    body[220:228] = "GGGGGGGG"                                # (matches none of the copy's last eight bases, TATTGCT + T... : low true scores)
    read = "".join(body)
    end_cells(read, ads, i0s, thetas, w, 0, 1 << 20, floors)
    assert fails(read, ads, i0s, thetas, w, 0, 1 << 20, floors, reset=False), "stale rows below r0 showed nowhere"
    # theta <= 0: plan() refuses it as row_skip_plan does (the column-0 condition); the header's own refusal is held by
    # tests/host/test_row_skip.cpp
    try:
        plan((Y28, Y22), 20, (58, 24))
    except AssertionError:
        pass
    else:
        raise AssertionError("theta = 0 accepted")
