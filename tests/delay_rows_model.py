"""CPU model of the delay-row layout of the dense HW read scan.

A read of m rows is laid into NWD 32-bit words bottom-aligned with R = 3 delay rows
below it: query row i sits at bit pad + i, pad = 32 NWD - R - m.  The pad bits below
row 0 and the R bits above row m-1 match every symbol.  A row that matches every
symbol copies the row above it one column late, so after a column j the top four bits
of Ph / Mh hold the bottom-row deltas of the columns j, j-1, j-2, j-3 (bit 28 .. 31 of
the last word), and the kernel moves the score once per group of four columns:

    score += popcount(Ph >> 28) - popcount(Mh >> 28)

Everything here is a Python-int Myers column (one long word of 32 NWD bits) written
the way scan_reads_kernel<NWD, 2, true, true> runs it; the tests set it against the
textbook DP.
"""
import numpy as np

R = 3            # delay rows
GROUP = 4        # columns per score update (kHitGroup)


def layout(m, nwd):
    """pad of a read of m rows in nwd words; ValueError when the layout does not fit."""
    pad = 32 * nwd - R - m
    if m < 1 or pad < 0:
        raise ValueError("a read of %d rows and %d delay rows does not fit %d words" % (m, R, nwd))
    return pad


def build_peq(query, nwd, nsym=4):
    """Peq rows as Python ints: bit pad + i of row s says query[i] == s; pads and delay rows match every symbol."""
    m = len(query)
    pad = layout(m, nwd)
    every = ((1 << pad) - 1) | (((1 << R) - 1) << (pad + m))
    rows = [every] * nsym
    for i, q in enumerate(query):
        rows[int(q)] |= 1 << (pad + i)
    return rows


def initial_state(m, nwd):
    """column -1: D[i][-1] = i + 1 on the query and delay rows, 0 on the pad rows."""
    W = 32 * nwd
    pad = layout(m, nwd)
    return ((1 << W) - 1) & ~((1 << pad) - 1), 0


def column(eq, pv, mv, W):
    """calculateBlock with hin = 0; returns the new state and this column's Ph, Mh BEFORE the shift."""
    full = (1 << W) - 1
    xv = eq | mv
    xh = ((((eq & pv) + pv) & full) ^ pv) | eq
    ph = (mv | ~(xh | pv)) & full
    mh = pv & xh
    phs = (ph << 1) & full
    mhs = (mh << 1) & full
    return (mhs | ~(xv | phs)) & full, phs & xv, ph, mh


def decode_group(score_before, nib_p, nib_m):
    """the slow path: per-column scores of a group from its nibbles (bit 3 = first column, bit 0 = last)."""
    out, s = [], score_before
    for b in (3, 2, 1, 0):
        s += ((nib_p >> b) & 1) - ((nib_m >> b) & 1)
        out.append(s)
    return out


def scan(query, target, nwd, start=0):
    """The kernel's loop from column `start` (a multiple of 16) to the end of the target.

    Returns (groups, tail): groups = [(last column, nibP, nibM, score after the update)], tail = [(column, score)] of the
    ragged columns past the last whole group of the last whole 16-column word, followed per column at bit 28.
    """
    assert start % 16 == 0
    m, W, T = len(query), 32 * nwd, len(target)
    peq = build_peq(query, nwd)
    pv, mv = initial_state(m, nwd)
    score = m
    groups, tail = [], []
    wend = T // 16 * 16
    j = start
    while j < wend:
        for q in range(GROUP):
            pv, mv, ph, mh = column(peq[int(target[j + q])], pv, mv, W)
        nib_p, nib_m = ph >> (W - 4), mh >> (W - 4)
        score += bin(nib_p).count("1") - bin(nib_m).count("1")
        groups.append((j + GROUP - 1, nib_p, nib_m, score))
        j += GROUP
    while j < T:
        pv, mv, ph, mh = column(peq[int(target[j])], pv, mv, W)
        score += ((ph >> (W - 4)) & 1) - ((mh >> (W - 4)) & 1)
        tail.append((j, score))
        j += 1
    return groups, tail


def dp_bottom_row(query, target):
    """Textbook HW DP: D[m-1][j] for every column j (row -1 is all zeros, column -1 is i + 1)."""
    q = np.asarray(query, dtype=np.int64)
    m = len(q)
    ramp = np.arange(1, m + 1, dtype=np.int64)
    col = ramp.copy()
    out = np.empty(len(target), dtype=np.int64)
    for j, t in enumerate(target):
        diag = np.concatenate(([0], col[:-1])) + (q != int(t))
        new = np.minimum(diag, col + 1)
        # vertical term: new[i] = min(new[i], new[i-1] + 1), with the zero row above row 0
        new = np.minimum(new, ramp)
        new = np.minimum.accumulate(new - ramp) + ramp
        col = new
        out[j] = col[-1]
    return out
