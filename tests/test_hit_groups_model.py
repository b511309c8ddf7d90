"""The group hit test of scan_reads_kernel (reads_kernels.hip) restated in numpy: after the columns of a group, one test of
the last score against best + G - 1; only a lane that passes it runs the per-column test on the group's columns, in order.
Scores of neighbouring columns differ by at most 1, so this must leave exactly the best, the count and the stored positions
(under a cap) of per-column tracking.  Groups of four (what the kernel uses) and of two."""
import itertools

import numpy as np
import pytest

CAP = 3          # small, so that walks of 8 columns overflow it


def track_columns(scores, best, cap=CAP, col0=0):
    """EDLIB_AMD_TRACK on every column: rows of `scores` are lanes"""
    n, L = scores.shape
    best = best.copy()
    cnt = np.zeros(n, dtype=np.int64)
    pos = np.full((n, cap), -1, dtype=np.int64)
    for j in range(L):
        s = scores[:, j]
        hit = s <= best
        better = s < best
        best = np.where(better, s, best)
        cnt = np.where(better, 0, cnt)
        st = hit & (cnt < cap)
        pos[np.nonzero(st)[0], cnt[st]] = col0 + j
        cnt = cnt + hit
    return best, cnt, pos


def track_groups(scores, best, G, cap=CAP):
    """the kernel's loop: full groups through the group test, the ragged rest column by column"""
    n, L = scores.shape
    best = best.copy()
    cnt = np.zeros(n, dtype=np.int64)
    pos = np.full((n, cap), -1, dtype=np.int64)
    slow = 0

    def columns(lanes, j0, j1):
        nonlocal best, cnt
        for j in range(j0, j1):
            s = scores[lanes, j]
            b, c = best[lanes], cnt[lanes]
            hit = s <= b
            better = s < b
            b = np.where(better, s, b)
            c = np.where(better, 0, c)
            st = hit & (c < cap)
            pos[lanes[st], c[st]] = j
            best[lanes], cnt[lanes] = b, c + hit
    full = L // G * G
    for j0 in range(0, full, G):
        lanes = np.nonzero(scores[:, j0 + G - 1] <= best + (G - 1))[0]
        slow += len(lanes)
        if len(lanes):
            columns(lanes, j0, j0 + G)
    columns(np.arange(n), full, L)
    return best, cnt, pos, slow


def _same(scores, best, G):
    want = track_columns(scores, best)
    got = track_groups(scores, best, G)
    for w, g, name in zip(want, got, ("best", "cnt", "pos")):
        assert np.array_equal(w, g), (G, name)
    return got[3]


@pytest.mark.parametrize("G", [4, 2])
def test_every_walk_of_8_columns(G):
    steps = np.array(list(itertools.product((-1, 0, 1), repeat=8)), dtype=np.int64)      # 6,561 walks
    best0 = 20
    for slack in range(6):                              # score of the column before the first, above best
        scores = best0 + slack + np.cumsum(steps, axis=1)
        slow = _same(scores, np.full(len(steps), best0, dtype=np.int64), G)
        assert 0 < slow < 8 // G * len(steps)           # both paths are taken


@pytest.mark.parametrize("G", [4, 2])
def test_walks_shorter_than_a_group_multiple(G):
    steps = np.array(list(itertools.product((-1, 0, 1), repeat=7)), dtype=np.int64)      # ragged rest of 3 (or 1) columns
    for slack in range(4):
        _same(10 + slack + np.cumsum(steps, axis=1), np.full(len(steps), 10, dtype=np.int64), G)


@pytest.mark.parametrize("G", [4, 2])
def test_random_walks_of_4096_columns_from_kinit_m(G):
    rng = np.random.default_rng(4100 + G)
    m = 150
    # column -1 scores m and kinit = m: the walk drifts down towards ~0.6 m and then hovers, as unrelated reads do
    steps = rng.choice((-1, 0, 1), size=(512, 4096), p=(0.3, 0.4, 0.3)).astype(np.int64)
    steps[:, :200] = rng.choice((-1, 0, 1), size=(512, 200), p=(0.5, 0.4, 0.1))
    scores = np.maximum(m + np.cumsum(steps, axis=1), 0)
    # clipping at 0 keeps steps within -1..1
    assert np.abs(np.diff(scores, axis=1)).max() <= 1
    slow = _same(scores, np.full(512, m, dtype=np.int64), G)
    assert slow < scores.size // G                       # most groups skip the per-column test
    # with room for every hit the stored positions are all of them
    want = track_columns(scores, np.full(512, m, dtype=np.int64), cap=64)
    got = track_groups(scores, np.full(512, m, dtype=np.int64), G, cap=64)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
