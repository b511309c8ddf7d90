"""The seven-delay-row layout of the dense HW read scan (tests/delay_rows8_model.py) against the textbook DP,
without a GPU: every read length that fits, for 1, 2, 5 and 8 words, against targets of 7, 8, 9, 19 and 100 random columns.

  (a) at every column j = 7 (mod 8) of a whole 16-column word the top byte of Ph / Mh is the eight bottom-row deltas of the
      columns j-7 .. j (bit 31 first);
  (b) the score after each group update (two popcounts) is the DP's;
  (c) the slow path's decode of the bytes gives the eight scores of the group;
  (d) the same for a scan restarted at a multiple of 16 after at least 2m - 1 warm-up columns;
  (e) a read of 32 NWD - 6 rows or more does not fit, and the selection rule takes 7, 7, 3, 3, 0 rows at
      m = 32 NWD - 8, - 7, - 6, - 3, - 2;
  (f) no column of a group scores below (before + after - 8) / 2, the scores before and after the group: the kernel's
      one-compare hit test per group -- over every one of the 3^8 delta sequences, over random scans, and over scans that
      hold an exact copy of the read (the score falls by 1 per column into the hit);
  (g) the tracking built on (f) and (c) leaves the best score, the count and the positions of a per-column test.
The ragged tail (columns past the last whole word, followed at bit 24) is checked with (b).
"""
import itertools

import numpy as np
import pytest

import delay_rows8_model as M

WORDS = (1, 2, 5, 8)
TARGETS = (7, 8, 9, 19, 100)
G = M.GROUP


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.int64)


def _check_scan(query, target, nwd, start, first):
    """columns >= first of a scan started at `start` against the DP over the whole target"""
    want = M.dp_bottom_row(query, target)
    m = len(query)
    groups, tail = M.scan(query, target, nwd, start)
    seen = 0
    for last, byte_p, byte_m, score in groups:
        if last - (G - 1) < first:
            continue
        before = int(want[last - G]) if last >= G else m
        deltas = [int(want[c]) - (int(want[c - 1]) if c >= 1 else m) for c in range(last - (G - 1), last + 1)]
        got = [((byte_p >> b) & 1) - ((byte_m >> b) & 1) for b in range(G - 1, -1, -1)]
        assert got == deltas, (m, nwd, last, got, deltas)                                     # (a)
        assert not (byte_p & byte_m) and byte_p < 256 and byte_m < 256, (m, nwd, last)
        assert score == int(want[last]), (m, nwd, last, score, int(want[last]))               # (b)
        assert M.decode_group(before, byte_p, byte_m) == [int(x) for x in want[last - (G - 1):last + 1]]   # (c)
        assert 2 * int(want[last - (G - 1):last + 1].min()) >= before + score - G             # (f)
        seen += G
    for col, score in tail:
        if col >= first:
            assert score == int(want[col]), (m, nwd, col, score, int(want[col]))
            seen += 1
    assert seen == len(target) - first
    return seen


@pytest.mark.parametrize("nwd", WORDS)
def test_byte_score_and_decode_at_every_length(nwd):
    rng = np.random.default_rng(9500 + nwd)
    for m in range(1, 32 * nwd - M.R + 1):
        query = _rand(rng, m)
        for T in TARGETS:
            _check_scan(query, _rand(rng, T), nwd, 0, 0)
        # a target that holds the read with one edit: the bottom row comes down to a small score and back
        target = _rand(rng, 100)
        if m <= 90:
            s = int(rng.integers(0, 100 - m + 1))
            target[s:s + m] = query
            target[s + m // 2] ^= 1
        _check_scan(query, target, nwd, 0, 0)


@pytest.mark.parametrize("nwd", WORDS)
def test_restart_after_warm_up(nwd):
    """(d): the segment [c0, T) from a scan that starts warm = 2 * 32 nwd - 1 columns earlier, rounded down to 16"""
    rng = np.random.default_rng(9600 + nwd)
    warm = 2 * 32 * nwd - 1
    for m in range(1, 32 * nwd - M.R + 1):
        assert warm >= 2 * (m + M.R) - 1
        query = _rand(rng, m)
        cw = 16 * int(rng.integers(1, 4))
        c0 = (cw + warm + 15) // 16 * 16
        T = c0 + 16 + int(rng.integers(0, 32))
        target = _rand(rng, T)
        e = int(rng.integers(c0, T))                         # a copy of the read that ends inside the segment
        lo = max(0, e - m + 1)
        target[lo:e + 1] = query[m - (e + 1 - lo):]
        assert ((c0 - warm) & ~15) == cw                     # the kernel's own rounding of the first warm-up column
        _check_scan(query, target, nwd, cw, c0)


@pytest.mark.parametrize("nwd", WORDS)
def test_reads_that_do_not_fit_and_the_selection_rule(nwd):
    """(e): the layout needs m + 7 <= 32 NWD; the last level takes seven rows, else three, else none"""
    M.layout(32 * nwd - 7, nwd)
    for m in range(32 * nwd - 6, 32 * nwd + 1):
        with pytest.raises(ValueError):
            M.layout(m, nwd)
        with pytest.raises(ValueError):
            M.build_peq(np.zeros(m, dtype=np.int64), nwd)
    picks = [M.rows_for(nwd, 32 * nwd - d) for d in (8, 7, 6, 3, 2)]
    assert picks == [7, 7, 3, 3, 0], picks
    assert M.rows_for(nwd, 32 * nwd - 1) == 0 and M.rows_for(nwd, 32 * nwd) == 0
    assert {M.rows_for(nwd, m) for m in range(1, 32 * nwd - 6)} == {7}
    assert {M.rows_for(nwd, m) for m in range(32 * nwd - 6, 32 * nwd - 2)} == {3}


def test_delay_rows_copy_the_bottom_row():
    """the identity itself: row m-1+d at column j holds the delta of row m-1 at column j-d, and -1 while j < d"""
    rng = np.random.default_rng(9700)
    nwd, m = 2, 40
    query, target = _rand(rng, m), _rand(rng, 60)
    want = M.dp_bottom_row(query, target)
    peq = M.build_peq(query, nwd)
    pv, mv = M.initial_state(m, nwd)
    pad = M.layout(m, nwd)
    for j in range(len(target)):
        pv, mv, ph, mh = M.column(peq[int(target[j])], pv, mv, 32 * nwd)
        for d in range(M.R + 1):
            got = ((ph >> (pad + m - 1 + d)) & 1) - ((mh >> (pad + m - 1 + d)) & 1)
            c = j - d
            exp = -1 if c < 0 else int(want[c]) - (int(want[c - 1]) if c >= 1 else m)
            assert got == exp, (j, d, got, exp)


def test_group_bound_over_every_delta_sequence():
    """(f) as a property of eight steps of -1, 0, +1: the least score is at least (a + b - 8) / 2, and the bound is met
    (a score falling 1 per column into a hit; four down and four up; eight level columns one above best are NOT passed)"""
    b = 50
    tight = 0
    for d in itertools.product((-1, 0, 1), repeat=G):
        sc = list(itertools.accumulate(d, initial=b))[1:]
        a = sc[-1]
        assert 2 * min(sc) >= a + b - G, d
        tight += 2 * min(sc) == a + b - G
        byte_p = sum(1 << (G - 1 - q) for q in range(G) if d[q] > 0)
        byte_m = sum(1 << (G - 1 - q) for q in range(G) if d[q] < 0)
        assert M.decode_group(b, byte_p, byte_m) == sc
        assert a == b + bin(byte_p).count("1") - bin(byte_m).count("1")
        # the test passes every group that holds a hit, whatever the threshold
        for best in range(min(sc) - 1, min(sc) + 2):
            if min(sc) <= best:
                assert M.may_hold_hit(b, a, best), (d, best)
    assert tight == 8                                                  # met by -1 x k then +1 x (8 - k), k = 1..8, only
    assert M.may_hold_hit(b, b - G, b - G) and M.may_hold_hit(b, b, b - 4)
    assert not M.may_hold_hit(b, b, b - 5) and not M.may_hold_hit(b - 3, b - 4, b - 8)


def _track_per_column(want, best, cap=16):
    cnt, pos = 0, []
    for col, sc in enumerate(want):
        sc = int(sc)
        if sc <= best:
            if sc < best:
                best, cnt, pos = sc, 0, []
            if cnt < cap:
                pos.append(col)
            cnt += 1
    return best, cnt, pos


@pytest.mark.parametrize("nwd", WORDS)
def test_tracking_equals_the_per_column_test(nwd):
    """(g): random reads, an exact copy ending at each of the eight places of a group (the score falls by 1 per column into
    the hit), a copy standing 20 times (the count runs past the cap of 16), two copies ending in one group"""
    rng = np.random.default_rng(9800 + nwd)
    m = 32 * nwd - M.R
    for trial in range(24):
        query = _rand(rng, m if trial % 2 else int(rng.integers(max(1, m - 24), m + 1)))
        mq = len(query)
        T = 16 * ((3 * mq + 400) // 16) + int(rng.integers(0, 16))
        if 8 <= trial < 12:
            T = 16 * (22 * mq // 16 + 1) + int(rng.integers(0, 16))
        target = _rand(rng, T)
        if trial < 8:                                                  # exact copy ending at place `trial` of its group
            e = 16 * ((mq + 40) // 16) + trial
            target[e - mq + 1:e + 1] = query
        elif trial < 12:                                               # the read repeated: a period of the target
            target = np.tile(query, 23)[:T]
        elif trial < 16 and mq >= 12:                                  # two ends in one group: the last symbol substituted
            e = 16 * ((mq + 40) // 16) + 1 + (trial - 12) * 2          # ... or left out: columns e - 1 and e both score 1
            target[e - mq + 1:e] = query[:-1]
            target[e] = query[-1] ^ 1
        want = M.dp_bottom_row(query, target)
        for best0 in (mq, int(want.min()), int(want.min()) + 3):
            got = M.track(query, target, nwd, best0)
            assert got == _track_per_column(want, best0), (nwd, trial, best0)
        got = M.track(query, target, nwd, mq)
        if trial < 8:
            assert got[0] == 0 and e in got[2] and e % G == trial
            assert mq < 20 or [int(x) for x in want[e - 5:e + 1]] == [5, 4, 3, 2, 1, 0]
        if 8 <= trial < 12:
            assert got[0] == 0 and got[1] >= 20 and len(got[2]) == 16
        if 12 <= trial < 16 and mq >= 12:
            assert got[0] == 1 and {e - 1, e} <= set(got[2]) and (e - 1) // G == e // G, (got, e)
