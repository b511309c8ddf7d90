"""The bottom-aligned layout of the dense last-level pass (scan_reads_kernel<NWD, 2, true>, build_peq_reads_kernel with
bottomAlign), as a long-integer model: the Myers column of calculateBlock (edlib.cpp:412-447) over one 32 NWD-bit word whose
low pad = 32 NWD - m bits are pad rows.  Query row r sits at bit pad + r, the pad bits of every symbol's row are set (a pad
row matches every symbol), and column -1 has Pv clear on the pad bits and set above them, Mv = 0.  In HW the pad rows stay
at D = 0 -- the boundary row the real rows always saw -- so the score followed at bit 32 NWD - 1, starting from m, is the
bottom row of the plain semi-global DP.  Checked against that DP for m = 1..160 at the word count of its group (every pad
0..31), for pads of whole words and more, and for targets that miss a symbol.  No GPU."""
import numpy as np
import pytest


def hw_bottom_row(q, t):
    """textbook DP, HW: D[-1][j] = 0, D[i][-1] = i + 1; the bottom row D[m-1][j] for every column j"""
    m = len(q)
    col = np.arange(1, m + 1, dtype=np.int64)
    out = np.empty(len(t), dtype=np.int64)
    for j, c in enumerate(t):
        new = np.empty_like(col)
        diag, up = 0, 0                                   # D[i-1][j-1], D[i-1][j] with i = 0: the zero row
        for i in range(m):
            v = min(diag + (0 if q[i] == c else 1), up + 1, col[i] + 1)
            diag = col[i]
            new[i] = up = v
        col = new
        out[j] = col[m - 1]
    return out


def peq_bottom(q, nwd, symbols):
    """what build_peq_reads_kernel writes with bottomAlign, the NWD words of a row as one integer"""
    m, pad = len(q), 32 * nwd - len(q)
    assert pad >= 0
    rows = {}
    for s in symbols:
        v = (1 << pad) - 1                                # pad rows match every symbol
        for r, c in enumerate(q):
            if c == s:
                v |= 1 << (pad + r)
        rows[s] = v
    return rows


def pv_words(m, nwd):
    """the initial Pv of scan_reads_kernel<NWD, 2, true>, word by word as the kernel computes it"""
    pad = 32 * nwd - m
    words = []
    for d in range(nwd):
        lo = pad - 32 * d
        words.append(0xFFFFFFFF if lo <= 0 else (0 if lo >= 32 else (0xFFFFFFFF << lo) & 0xFFFFFFFF))
    return words


def scan_bottom(q, t, nwd, symbols):
    """bottom-row scores of every column by the bottom-aligned Myers column (HW: hin = 0)"""
    m, W = len(q), 32 * nwd
    pad, full = W - m, (1 << W) - 1
    peq = peq_bottom(q, nwd, symbols)
    pv = full ^ ((1 << pad) - 1)
    assert pv == sum(w << (32 * d) for d, w in enumerate(pv_words(m, nwd)))
    mv, score = 0, m
    out = np.empty(len(t), dtype=np.int64)
    for j, c in enumerate(t):
        eq = peq[c]
        xv = eq | mv
        xh = ((((eq & pv) + pv) & full) ^ pv) | eq
        ph = mv | (full & ~(xh | pv))
        mh = pv & xh
        score += (ph >> (W - 1)) & 1                      # v_lshrrev_b32 31
        score -= (mh >> (W - 1)) & 1                      # v_ashrrev_i32 31
        ph = (ph << 1) & full                             # row -1 of HW: a zero comes in
        mh = (mh << 1) & full
        pv = mh | (full & ~(xv | ph))
        mv = ph & xv
        assert pv & ((1 << pad) - 1) == 0 and mv & ((1 << pad) - 1) == 0     # the pad rows stay at D = 0
        out[j] = score
    return out


def scan_bottom_words(q, t, nwd, symbols):
    """the same column on NWD 32-bit words, instruction by instruction as reads_column_asm.hpp has it: the v_add_co /
    v_addc_co chain, word 0 shifted by an add (a zero comes in), the others by v_alignbit_b32 with the word below, the score
    from bit 31 of the last word's deltas (v_lshrrev_b32 / v_ashrrev_i32 by 31)"""
    M32 = 0xFFFFFFFF
    m = len(q)
    peq = {s: [(v >> (32 * d)) & M32 for d in range(nwd)] for s, v in peq_bottom(q, nwd, symbols).items()}
    pv, mv, score = pv_words(m, nwd), [0] * nwd, m
    out = np.empty(len(t), dtype=np.int64)
    for j, c in enumerate(t):
        e = peq[c]
        cy, ph, mh, pn, mn = 0, [0] * nwd, [0] * nwd, [0] * nwd, [0] * nwd
        for i in range(nwd):
            s = (e[i] & pv[i]) + pv[i] + cy
            cy, s = s >> 32, s & M32
            xh = (s ^ pv[i]) | e[i]
            ph[i] = mv[i] | (M32 & ~(xh | pv[i]))
            mh[i] = pv[i] & xh
            phs = (ph[0] + ph[0]) & M32 if i == 0 else ((ph[i] << 1) & M32) | (ph[i - 1] >> 31)
            mhs = (mh[0] + mh[0]) & M32 if i == 0 else ((mh[i] << 1) & M32) | (mh[i - 1] >> 31)
            xv = e[i] | mv[i]
            pn[i] = mhs | (M32 & ~(xv | phs))
            mn[i] = phs & xv
        score += (ph[nwd - 1] >> 31) - (mh[nwd - 1] >> 31)
        pv, mv = pn, mn
        out[j] = score
    return out


def _case(rng, m, nwd, T, tsyms=4):
    q = rng.integers(0, 4, m).tolist()
    t = rng.integers(0, tsyms, T).tolist()
    if m >= 6 and T > m + 10:                             # a related window, so that low scores occur as well
        s = int(rng.integers(0, T - m))
        w = list(q)
        for _ in range(int(rng.integers(0, 1 + m // 6))):
            w[int(rng.integers(0, m))] = int(rng.integers(0, tsyms))
        t[s:s + m] = w
        if tsyms < 4:
            t = [min(c, tsyms - 1) for c in t]
    return q, t


@pytest.mark.parametrize("m0", range(1, 161, 16))
def test_every_length_at_its_groups_word_count(m0):
    """m = 1..160 in the group that holds it: the pads 0..31 at one to five words"""
    rng = np.random.default_rng(900 + m0)
    pads = set()
    for m in range(m0, m0 + 16):
        nwd = (m + 31) // 32
        pads.add(32 * nwd - m)
        q, t = _case(rng, m, nwd, 2 * m + 40)
        assert np.array_equal(scan_bottom(q, t, nwd, range(4)), hw_bottom_row(q, t)), m
    assert len(pads) == 16


@pytest.mark.parametrize("nwd", range(1, 9))
def test_word_level_column_is_the_long_integer_one(nwd):
    rng = np.random.default_rng(9500 + nwd)
    for m in sorted({1, max(1, 32 * nwd - 63), 32 * nwd - 31, 32 * nwd - 20, 32 * nwd - 1, 32 * nwd}):
        q, t = _case(rng, m, nwd, 2 * m + 40)
        want = hw_bottom_row(q, t)
        assert np.array_equal(scan_bottom_words(q, t, nwd, range(4)), want), (m, nwd)
        assert np.array_equal(scan_bottom(q, t, nwd, range(4)), want), (m, nwd)


def test_all_pads_below_a_word_occur():
    assert {32 * ((m + 31) // 32) - m for m in range(1, 161)} == set(range(32))


@pytest.mark.parametrize("m,nwd", [(1, 2), (1, 5), (1, 8), (7, 3), (32, 2), (33, 3), (40, 4), (64, 5), (100, 8), (129, 8)])
def test_pads_of_a_word_and_more(m, nwd):
    """a read shorter than its group's last word reaches (the padding slots of a rebuilt list have m = 1): whole pad words"""
    assert 32 * nwd - m >= 32
    rng = np.random.default_rng(7000 + 10 * m + nwd)
    for _ in range(3):
        q, t = _case(rng, m, nwd, 2 * m + 50)
        assert np.array_equal(scan_bottom(q, t, nwd, range(4)), hw_bottom_row(q, t))


@pytest.mark.parametrize("tsyms", [1, 2, 3])
def test_target_missing_symbols(tsyms):
    """the query holds symbols the target never shows: their rows are never picked, the pad bits of the others still are"""
    rng = np.random.default_rng(8100 + tsyms)
    for m in (1, 5, 31, 32, 33, 95, 129, 150, 160):
        for nwd in {(m + 31) // 32, min(8, (m + 31) // 32 + 1)}:
            q, t = _case(rng, m, nwd, 2 * m + 30, tsyms)
            assert max(t) < tsyms
            assert np.array_equal(scan_bottom(q, t, nwd, range(tsyms)), hw_bottom_row(q, t)), (m, nwd)
