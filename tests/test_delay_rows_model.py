"""The delay-row layout of the dense HW read scan (tests/delay_rows_model.py) against the textbook DP, without
a GPU: every read length that fits, for 1, 2, 5 and 8 words, against targets of 3, 4, 5, 19 and 100 random columns.

  (a) at every column j = 3 (mod 4) of a whole 16-column word the top nibble of Ph / Mh is the four bottom-row deltas of the
      columns j-3 .. j (bit 31 first);
  (b) the score after each group update is the DP's;
  (c) the slow path's decode of the nibbles gives the four scores of the group;
  (d) the same for a scan restarted at a multiple of 16 after at least 2m - 1 warm-up columns;
  (e) a read of 32 NWD - 2 rows or more does not fit: the eligibility rule of engine_reads.hip;
  (f) no column of a group scores below (before + after - 4) / 2, the scores before and after the group: the kernel's
      one-compare hit test per group.
The ragged tail (columns past the last whole word, followed at bit 28) is checked with (b).
"""
import numpy as np
import pytest

import delay_rows_model as M

WORDS = (1, 2, 5, 8)
TARGETS = (3, 4, 5, 19, 100)


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.int64)


def _check_scan(query, target, nwd, start, first):
    """columns >= first of a scan started at `start` against the DP over the whole target"""
    want = M.dp_bottom_row(query, target)
    m = len(query)
    groups, tail = M.scan(query, target, nwd, start)
    seen = 0
    for last, nib_p, nib_m, score in groups:
        if last - 3 < first:
            continue
        before = int(want[last - 4]) if last >= 4 else m
        deltas = [int(want[c]) - (int(want[c - 1]) if c >= 1 else m) for c in range(last - 3, last + 1)]
        got = [((nib_p >> b) & 1) - ((nib_m >> b) & 1) for b in (3, 2, 1, 0)]
        assert got == deltas, (m, nwd, last, got, deltas)                                     # (a)
        assert not (nib_p & nib_m), (m, nwd, last)
        assert score == int(want[last]), (m, nwd, last, score, int(want[last]))               # (b)
        assert M.decode_group(before, nib_p, nib_m) == [int(x) for x in want[last - 3:last + 1]]   # (c)
        assert 2 * int(want[last - 3:last + 1].min()) >= before + score - 4                  # (f)
        seen += 4
    for col, score in tail:
        if col >= first:
            assert score == int(want[col]), (m, nwd, col, score, int(want[col]))
            seen += 1
    assert seen == len(target) - first
    return seen


@pytest.mark.parametrize("nwd", WORDS)
def test_nibble_score_and_decode_at_every_length(nwd):
    rng = np.random.default_rng(9100 + nwd)
    for m in range(1, 32 * nwd - M.R + 1):
        query = _rand(rng, m)
        for T in TARGETS:
            _check_scan(query, _rand(rng, T), nwd, 0, 0)
        # a target that holds the read with a few edits: the bottom row comes down to a small score and back
        target = _rand(rng, 100)
        if m <= 90:
            s = int(rng.integers(0, 100 - m + 1))
            target[s:s + m] = query
            target[s + m // 2] ^= 1
        _check_scan(query, target, nwd, 0, 0)


@pytest.mark.parametrize("nwd", WORDS)
def test_restart_after_warm_up(nwd):
    """(d): the segment [c0, T) from a scan that starts warm = 2 * 32 nwd - 1 columns earlier, rounded down to 16"""
    rng = np.random.default_rng(9200 + nwd)
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
def test_reads_that_do_not_fit(nwd):
    """(e): the layout needs m + 3 <= 32 NWD"""
    M.layout(32 * nwd - 3, nwd)
    for m in (32 * nwd - 2, 32 * nwd - 1, 32 * nwd):
        with pytest.raises(ValueError):
            M.layout(m, nwd)
        with pytest.raises(ValueError):
            M.build_peq(np.zeros(m, dtype=np.int64), nwd)


def test_delay_rows_copy_the_bottom_row():
    """the identity itself: row m-1+d at column j holds the delta of row m-1 at column j-d, and -1 while j < d"""
    rng = np.random.default_rng(9300)
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
