"""The 2 x 2 blocked column pair of the specialised score kernel (csrc/pc_jit_source.h, column2, packed fp16) against the
plain five-op recurrence, as a numpy model -- no GPU, no library.

Both run in the kernel's drifted frame (X~ = X + (rho + jj) * eps - C, T one step ahead) on float64 arrays that hold
integers and the real -infinity, as the fp16 lanes do.  The blocked model forms exactly the maxima the kernel's asm
statements form, unit by unit (row pairs, an odd last row as an even-type row on its own):

    chain A (column j)    Vb  = max3(Vb, T(e-2,j), T(e-1,j))          M(e,j)   = max3(d, U[e], Vb)
                                                                      M(o,j)   = max(max3(d, U[o], Vb), T(e,j))
    chain B (column j+1)  Vb' = max3(Vb', T(e-2,j+1), T(e-1,j+1))     M(e,j+1) = max(max3(d', U[e], T(e,j)), Vb')
                                                                      M(o,j+1) = max3(max3(d', U[o], T(o,j)), Vb', T(e,j+1))
                          U[.] = max3(U[.], T(.,j), T(.,j+1))

with U[rho] = H(rho, j) of the coming column (the plain recurrence: H(rho, j-1)).  A schedule mixes single columns (the
one-column path, which is the plain recurrence on the shared state) with column pairs, converts U on every entry into a
pair stretch, and renormalises in between.  Every T, every H (as the blocked scheme implies it: U for column j,
max(U, T(., j)) for column j+1), the V of the even rows (the only ones materialised) and every tracked last-row term
`cand` must equal the plain recurrence's, cell for cell."""
import random

import numpy as np
import pytest

NEG = -np.inf
MATCH, MISMATCH, OPEN, EXT = 3, -6, -5, -2
EPS = -EXT
OE = OPEN + EPS
CEN = 7                      # any centring constant: both models share it
DK = 12 * EPS                # what a renormalisation subtracts (the kernel: PC_KREN * eps)


def max3(a, b, c):
    return np.maximum(np.maximum(a, b), c)


def sub_terms(adapter, col_bases):
    """S~[rho, lane] of one column: sub - open + eps."""
    ad = np.array(list(adapter))[:, None]
    return np.where(ad == col_bases[None, :], MATCH, MISMATCH).astype(np.float64) - OPEN + EPS


def initial_state(R, lanes):
    T = np.repeat((OPEN + (np.arange(R) + 2) * EPS - CEN).astype(np.float64)[:, None], lanes, axis=1)
    U = np.full((R, lanes), NEG)
    top = np.full(lanes, float(OPEN + EPS - CEN))
    return T, U, top


def plain_column(T, U, top, S):
    """The five-op recurrence.  -> new (T, U, top), and per cell H, V, cand."""
    R = T.shape[0]
    topn = top + EPS
    Tn, H, V = np.empty_like(T), np.empty_like(T), np.empty_like(T)
    vprev, tup = np.full_like(top, NEG), topn
    for r in range(R):
        H[r] = np.maximum(U[r], T[r])
        V[r] = np.maximum(vprev, tup)
        d = (top if r == 0 else T[r - 1]) + S[r]
        Tn[r] = max3(d, H[r], V[r]) + OE
        vprev, tup = V[r], Tn[r]
    return Tn, H, topn, H.copy(), V, Tn[R - 1] - topn


def blocked_pair(T, U, top, S1, S2):
    """Two columns, 2 x 2 blocked; U enters and leaves as the H of the coming column.
    -> new (T, U, top), and per column (T, H, V of the even rows, cand)."""
    R = T.shape[0]
    topA, topB = top + EPS, top + 2 * EPS
    TA, TB, Un = np.empty_like(T), np.empty_like(T), np.empty_like(U)
    VA, VB = {}, {}
    vbA = vbB = np.full_like(top, NEG)
    for e in range(0, R, 2):
        o = e + 1
        # chain A
        vbA = max3(vbA, TA[e - 2] if e else np.full_like(top, NEG), TA[e - 1] if e else topA)
        VA[e] = vbA
        dA = (top if e == 0 else T[e - 1]) + S1[e]
        TA[e] = max3(dA, U[e], vbA) + OE
        if o < R:
            TA[o] = np.maximum(max3(T[e] + S1[o], U[o], vbA), TA[e]) + OE
    for f in range(0, R, 2):
        g = f + 1
        # chain B
        vbB = max3(vbB, TB[f - 2] if f else np.full_like(top, NEG), TB[f - 1] if f else topB)
        VB[f] = vbB
        dB = (topA if f == 0 else TA[f - 1]) + S2[f]
        TB[f] = np.maximum(max3(dB, U[f], TA[f]), vbB) + OE
        Un[f] = max3(U[f], TA[f], TB[f])
        if g < R:
            TB[g] = max3(max3(TA[f] + S2[g], U[g], TA[g]), vbB, TB[f]) + OE
            Un[g] = max3(U[g], TA[g], TB[g])
    colA = (TA, U.copy(), VA, TA[R - 1] - topA)
    colB = (TB, np.maximum(U, TA), VB, TB[R - 1] - topB)
    return TB, Un, topB, colA, colB


def run_plain(adapter, reads, renorm_before):
    R, n = len(adapter), reads.shape[1]
    T, U, top = initial_state(R, reads.shape[0])
    cells = []
    for j in range(n):
        if j in renorm_before:
            T, U, top = T - DK, U - DK, top - DK
        T, U, top, H, V, cand = plain_column(T, U, top, sub_terms(adapter, reads[:, j]))
        cells.append((T, H, V, cand))
    return cells


def run_blocked(adapter, reads, schedule, renorm_before):
    """schedule: a list of 1s and 2s that sums to the number of columns."""
    R = len(adapter)
    T, U, top = initial_state(R, reads.shape[0])
    cells, j, u_ahead = [], 0, False
    for step in schedule:
        if j in renorm_before:
            T, U, top = T - DK, U - DK, top - DK
        if step == 2:
            if not u_ahead:                                   # the entry conversion
                U, u_ahead = np.maximum(U, T), True
            T, U, top, colA, colB = blocked_pair(T, U, top, sub_terms(adapter, reads[:, j]), sub_terms(adapter, reads[:, j + 1]))
            cells += [colA, colB]
        else:
            u_ahead = False                                   # the one-column path needs no conversion: max(U, T) is U
            T, U, top, H, V, cand = plain_column(T, U, top, sub_terms(adapter, reads[:, j]))
            cells.append((T, H, {r: V[r] for r in range(R)}, cand))
        j += step
    return cells


def make_reads(rng, adapter, n, lanes=24):
    R = len(adapter)
    rows = []
    for k in range(lanes):
        kind = k % 4
        if kind == 0:
            r = [rng.choice("ACGT") for _ in range(n)]
        elif kind == 1:                                       # a long horizontal gap: the adapter with many read bases in its middle
            cut, gap = R // 2, rng.randint(6, 12)
            r = list(adapter[:cut]) + [rng.choice("ACGT") for _ in range(gap)] + list(adapter[cut:])
        elif kind == 2:                                       # a long vertical gap: the adapter with its middle missing
            keep = max(1, R // 4)
            r = list(adapter[:keep]) + list(adapter[R - keep:])
        else:                                                 # a clean copy somewhere
            r = [rng.choice("ACGT") for _ in range(rng.randint(0, 3))] + list(adapter)
        r = (r + [rng.choice("ACGT") for _ in range(n)])[:n]
        rows.append(r)
    return np.array(rows)


def schedules(rng, n):
    out = [[2] * (n // 2) + [1] * (n % 2),                    # pairs from the first column
           [1] + [2] * ((n - 1) // 2) + [1] * ((n - 1) % 2)]  # entered at an even column
    alt, left, step = [], n, 2                                # pair, single, pair, ...: left and re-entered at both parities
    while left:
        s = min(step, left)
        alt.append(s); left -= s; step = 3 - step
    out.append(alt)
    for _ in range(3):
        sc, left = [], n
        while left:
            s = rng.choice([1, 2, 2]) if left >= 2 else 1
            sc.append(s); left -= s
        out.append(sc)
    return out


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 28, 33])
def test_blocked_column_pairs_equal_the_plain_recurrence(R):
    rng = random.Random(100 + R)
    checked_entries = checked_mid_renorm = 0
    for n in list(range(1, 10)) + [40]:
        adapter = "".join(rng.choice("ACGT") for _ in range(R))
        reads = make_reads(rng, adapter, n)
        for sc in schedules(rng, n):
            starts = np.cumsum([0] + sc[:-1]).tolist()
            # renormalise before some steps; always once between two pairs where the schedule has two in a row
            renorm = {s for s in starts if s and rng.random() < 0.25}
            for a, b, s in zip(sc, sc[1:], starts[1:]):
                if a == 2 and b == 2:
                    renorm.add(s); checked_mid_renorm += 1
                    break
            checked_entries += sum(1 for a, b in zip([1] + sc, sc) if a == 1 and b == 2)
            want = run_plain(adapter, reads, renorm)
            got = run_blocked(adapter, reads, sc, renorm)
            assert len(got) == len(want) == n
            for j, ((Tw, Hw, Vw, cw), (Tg, Hg, Vg, cg)) in enumerate(zip(want, got)):
                where = (R, n, sc, sorted(renorm), j)
                assert np.array_equal(Tg, Tw), where
                assert np.array_equal(Hg, Hw), where
                assert np.array_equal(cg, cw), where
                assert Vg and all(np.array_equal(v, Vw[r]) for r, v in Vg.items()), where
                assert all(r in Vg for r in range(0, R, 2)), where
    assert checked_entries > 10 and checked_mid_renorm >= 4, (checked_entries, checked_mid_renorm)


def test_the_models_see_gaps_and_minus_infinity():
    """The inputs do what they are for: somewhere H wins a cell, somewhere V wins, and U starts at -infinity."""
    rng = random.Random(7)
    adapter = "".join(rng.choice("ACGT") for _ in range(28))
    reads = make_reads(rng, adapter, 40)
    cells = run_plain(adapter, reads, set())
    T0, U0, _ = initial_state(28, reads.shape[0])
    assert np.isneginf(U0).all()
    h_wins = v_wins = 0
    for j, (T, H, V, cand) in enumerate(cells):
        M = T - OE
        h_wins += int(((H == M) & (V < M)).sum())
        v_wins += int(((V == M) & (H < M)).sum())
    assert h_wins > 0 and v_wins > 0, (h_wins, v_wins)
