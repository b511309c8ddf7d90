"""tests/shared_best_model.py against the textbook DP: whatever the segments of a read import, and whenever, the merged
(best, count, first 16 positions, overflow flag) is the DP's, as long as no import is below the read's true minimum."""
import numpy as np
import pytest

import shared_best_model as SB
from delay_rows_model import dp_bottom_row


def _case(seed, m=24, T=1501, copies=(), edits=3, period=0):
    """a random target with the read's window planted at `copies` (each with `edits` substitutions of its own); period > 0:
    a periodic stretch instead, where the read ties every `period` columns"""
    rng = np.random.default_rng(seed)
    target = rng.integers(0, 4, T)
    if period:
        unit = rng.integers(0, 4, period)
        span = m + period * 24
        target[300:300 + span] = np.resize(unit, span)
        query = np.resize(unit, m).copy()
        query[::5] = (query[::5] + 1) % 4
        return query, target
    query = rng.integers(0, 4, m)
    for at in copies:
        w = query.copy()
        for p in rng.choice(m, edits, replace=False):
            w[p] = (w[p] + 1 + rng.integers(0, 3)) % 4
        target[at:at + m] = w
    return query, target


def _segments(T, S):
    seg_len, S = SB.plan(T, S)
    return [(s * seg_len, min(T, (s + 1) * seg_len)) for s in range(S)]


def _own_hits(query, target, S):
    """per segment: the columns that score the segment's own minimum"""
    row = dp_bottom_row(query, target)
    out = []
    for c0, c1 in _segments(len(target), S):
        part = row[c0:c1]
        out.append([c0 + int(i) for i in np.flatnonzero(part == part.min())])
    return row, out


CASES = {
    "last_only": dict(seed=1, copies=(1430,), edits=2),                       # the minimum occurs only in the last segment
    "tie_first_last": dict(seed=2, copies=(40, 1440), edits=0),               # the same window in the first and the last
    "better_later": dict(seed=3, copies=(60,), edits=6),                      # (a second, better copy is added below)
    "many_ties": dict(seed=4, period=7),                                      # more than 16 equal hits in one segment
    "ragged_tail": dict(seed=5, copies=(1501 - 24,), edits=1),                # the hit is the last column
    "random": dict(seed=6),
}


def _build(name):
    q, t = _case(**CASES[name])
    if name == "better_later":
        t[900:900 + len(q)] = q
        t[910] = (t[910] + 1) % 4
    return q, t


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_imports_is_the_textbook(name):
    q, t = _build(name)
    for S in (1, 3, 5):
        assert SB.run(q, t, S, {}) == SB.textbook(q, t)


def test_the_cases_are_what_they_say():
    q, t = _build("last_only")
    row, own = _own_hits(q, t, 5)
    segs = _segments(len(t), 5)
    assert all(c >= segs[-1][0] for c in np.flatnonzero(row == row.min()))
    q, t = _build("tie_first_last")
    row = dp_bottom_row(q, t)
    hits = np.flatnonzero(row == row.min())
    assert hits[0] < segs[0][1] and hits[-1] >= segs[-1][0]
    q, t = _build("better_later")
    row = dp_bottom_row(q, t)
    assert row[:segs[0][1]].min() > row.min() and row[:segs[0][1]].min() < len(q) // 2
    q, t = _build("many_ties")
    b, n, pos, ovf = SB.textbook(q, t)
    assert n > 16 and ovf and len({next(i for i, (c0, c1) in enumerate(segs) if c0 <= p < c1) for p in pos}) == 1
    q, t = _build("ragged_tail")
    row = dp_bottom_row(q, t)
    assert list(np.flatnonzero(row == row.min())) == [len(t) - 1] and len(t) % 16 != 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_minimum_before_at_and_after_own_hits(name):
    """every segment is handed the read's true minimum just before its first own hit, at each own hit, right after it, at
    its first column and past its last one -- one delivery per run, and all of them together"""
    q, t = _build(name)
    want = SB.textbook(q, t)
    S = 5
    row, own = _own_hits(q, t, S)
    gmin = int(row.min())
    segs = _segments(len(t), S)
    for s, (c0, c1) in enumerate(segs):
        cols = {c0, c1 + 5}
        for h in own[s][:3] + own[s][-2:]:
            cols.update(c for c in (h - 1, h, h + 1) if c >= c0)
        for c in sorted(cols):
            assert SB.run(q, t, S, {s: [(c, gmin)]}) == want, (name, s, c)
        assert SB.run(q, t, S, {s: [(c, gmin) for c in sorted(cols)]}) == want, (name, s)
    everywhere = {s: [(c, gmin) for c in range(c0, c1, 16)] for s, (c0, c1) in enumerate(segs)}
    assert SB.run(q, t, S, everywhere) == want


@pytest.mark.parametrize("name", sorted(CASES))
def test_bounds_between_the_minimum_and_the_threshold(name):
    """imports of gmin, gmin + 1, ... in falling and rising order, and the start itself at every value down to gmin"""
    q, t = _build(name)
    want = SB.textbook(q, t)
    S = 5
    gmin = want[0]
    segs = _segments(len(t), S)
    falling = {s: [(c0 + 16 * i, max(gmin, len(q) - i)) for i in range((c1 - c0) // 16)] for s, (c0, c1) in enumerate(segs)}
    assert SB.run(q, t, S, falling) == want
    rising = {s: [(c0 + 16 * i, gmin + i) for i in range((c1 - c0) // 16)] for s, (c0, c1) in enumerate(segs)}
    assert SB.run(q, t, S, rising) == want
    for start in range(gmin, len(q) + 1):
        assert SB.run(q, t, S, {}, start=start) == want, start


@pytest.mark.parametrize("seed", range(12))
def test_random_schedules(seed):
    rng = np.random.default_rng(100 + seed)
    name = sorted(CASES)[seed % len(CASES)]
    q, t = _build(name)
    want = SB.textbook(q, t)
    S = int(rng.integers(2, 9))
    segs = _segments(len(t), S)
    for _ in range(6):
        sched = {}
        for s, (c0, c1) in enumerate(segs):
            n = int(rng.integers(0, 12))
            sched[s] = [(int(rng.integers(c0, c1 + 3)), int(rng.integers(want[0], len(q) + 1))) for _ in range(n)]
        assert SB.run(q, t, S, sched) == want, sched


def test_published_values_in_any_order():
    """the real thing: segments run one after the other in a random order, each starts from and imports only what the
    ones before it published (their own bests), at its first column and at one column in the middle"""
    rng = np.random.default_rng(7)
    for name in sorted(CASES):
        q, t = _build(name)
        want = SB.textbook(q, t)
        S = 6
        segs = _segments(len(t), S)
        for _ in range(4):
            shared = len(q)
            records = [None] * len(segs)
            for s in rng.permutation(len(segs)):
                c0, c1 = segs[s]
                rec = SB.scan_segment(SB.segment_scores(q, t, c0, c1, 2 * len(q) - 1), c0, len(q),
                                      [(c0, shared), ((c0 + c1) // 2, shared)])
                records[s] = rec
                if rec[1] > 0:
                    shared = min(shared, rec[0])
            assert SB.merge(records) == want, name


def test_a_bound_below_the_minimum_is_what_breaks_it():
    """the premise is needed: an import below every score leaves nothing to merge"""
    q, t = _build("random")
    got = SB.run(q, t, 3, {s: [(0, -1)] for s in range(3)}, start=-1)
    assert got == (-1, 0, [], False) and got != SB.textbook(q, t)
