"""CPU model of the seven-delay-row layout of the dense HW read scan, the deeper of the two depths.

A read of m rows is laid into NWD 32-bit words bottom-aligned with R = 7 delay rows
above row m-1: query row i sits at bit pad + i, pad = 32 NWD - R - m.  The pad bits below
row 0 and the R bits above row m-1 match every symbol.  A row that matches every
symbol copies the row above it one column late, so after a column j the top byte
of Ph / Mh holds the bottom-row deltas of the columns j, j-1, ..., j-7 (bit 24 .. 31 of
the last word), and the kernel moves the score once per group of eight columns:

    score += popcount(Ph >> 24) - popcount(Mh >> 24)

Everything here is a Python-int Myers column (one long word of 32 NWD bits) written
the way scan_reads_kernel<NWD, 2, true, 7> runs it; the tests set it against the
textbook DP.  The column and the DP are those of tests/delay_rows_model.py (depth 3).
"""
from delay_rows_model import column, dp_bottom_row    # noqa: F401  (the same recurrence and reference at both depths)

R = 7            # delay rows
GROUP = 8        # columns per score update and hit test (kHitGroup = R + 1)
DEPTHS = (7, 3)  # what a group may carry, deepest first (engine_reads.hip)


def rows_for(nwd, longest):
    """the selection rule of the last level: seven rows where the group's longest read leaves them room, else three, else 0"""
    for r in DEPTHS:
        if 1 <= longest and longest + r <= 32 * nwd:
            return r
    return 0


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


def decode_group(score_before, byte_p, byte_m):
    """the slow path: per-column scores of a group from its bytes (bit 7 = first column, bit 0 = last)."""
    out, s = [], score_before
    for b in range(GROUP - 1, -1, -1):
        s += ((byte_p >> b) & 1) - ((byte_m >> b) & 1)
        out.append(s)
    return out


def may_hold_hit(score_before, score_after, best):
    """the kernel's one compare per group: a + b <= 2 best + 8 (lim2)"""
    return score_before + score_after <= 2 * best + GROUP


def scan(query, target, nwd, start=0):
    """The kernel's loop from column `start` (a multiple of 16) to the end of the target.

    Returns (groups, tail): groups = [(last column, byteP, byteM, score after the update)], tail = [(column, score)] of the
    ragged columns past the last whole 16-column word, followed per column at bit 24.
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
        byte_p, byte_m = ph >> (W - GROUP), mh >> (W - GROUP)
        score += bin(byte_p).count("1") - bin(byte_m).count("1")
        groups.append((j + GROUP - 1, byte_p, byte_m, score))
        j += GROUP
    while j < T:
        pv, mv, ph, mh = column(peq[int(target[j])], pv, mv, W)
        score += ((ph >> (W - GROUP)) & 1) - ((mh >> (W - GROUP)) & 1)
        tail.append((j, score))
        j += 1
    return groups, tail


def track(query, target, nwd, best, cap=16):
    """The kernel's tracking over one segment [0, T) from the threshold `best`: the group test, the decode, the per-column
    test only where the least score of the group is a hit.  Returns (best, count, positions), what EDLIB_AMD_TRACK_SCORE leaves."""
    m = len(query)
    groups, tail = scan(query, target, nwd)
    cnt, pos, before = 0, [], m

    def hit(sc, col):
        nonlocal best, cnt, pos
        if sc <= best:
            if sc < best:
                best, cnt, pos = sc, 0, []
            if cnt < cap:
                pos.append(col)
            cnt += 1

    for last, bp, bm, score in groups:
        if may_hold_hit(before, score, best):
            sc = decode_group(before, bp, bm)
            if min(sc) <= best:
                for q, s in enumerate(sc):
                    hit(s, last - (GROUP - 1) + q)
        before = score
    for col, score in tail:
        hit(score, col)
    return best, cnt, pos
