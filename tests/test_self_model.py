"""CPU: the host statements of a self batch's layout and rules -- condensed_index() against brute-force enumeration (and
scipy's squareform where scipy is installed), self_nearest_model() on hand-made lists, and the counters of a self batch
(cells, word_steps) as numpy functions that the GPU tests use again."""
import numpy as np
import pytest

import edlib_amd

KERNEL_MAX = 256          # bases of a sequence the self kernel takes (longer ones: the internal pair batch)


def self_cells(lengths):
    """Stats.cells of a self batch: the sum of m_i * m_j over i < j."""
    m = np.asarray(lengths, dtype=object)
    return int((m.sum() ** 2 - (m * m).sum()) // 2) if len(m) else 0


def self_word_steps(lengths, k):
    """Stats.word_steps of a self batch over at most 16 symbols: the sum of ceil(min / 32) * max of the two lengths over
    the pairs i < j the kernel scans -- both sequences with bases, neither above 256, lengths within k of each other
    (any pair for k < 0)."""
    m = np.asarray(lengths, dtype=np.int64)
    m = m[(m > 0) & (m <= KERNEL_MAX)]
    i, j = np.triu_indices(len(m), 1)
    lo, hi = np.minimum(m[i], m[j]), np.maximum(m[i], m[j])
    inside = np.ones(len(lo), dtype=bool) if k < 0 else (hi - lo <= k)
    return int((((lo + 31) // 32) * hi)[inside].sum())


@pytest.mark.parametrize("n", [0, 1, 2, 3, 65])
def test_condensed_index_enumerates_the_triangle(n):
    at = 0
    for i in range(n):
        for j in range(i + 1, n):
            assert edlib_amd.condensed_index(n, i, j) == at
            assert edlib_amd.condensed_index(n, j, i) == at
            at += 1
    assert at == n * (n - 1) // 2
    i, j = np.triu_indices(n, 1)
    got = edlib_amd.condensed_index(n, i, j)
    assert np.array_equal(got, np.arange(n * (n - 1) // 2))


def test_condensed_index_is_64_bit():
    n = 200_000
    assert edlib_amd.condensed_index(n, n - 2, n - 1) == n * (n - 1) // 2 - 1
    assert edlib_amd.condensed_index(n, 100_000, 150_000) == n * 100_000 - 100_000 * 100_001 // 2 + 49_999


def test_condensed_index_matches_squareform():
    distance = pytest.importorskip("scipy.spatial.distance")
    for n in (2, 3, 65):
        v = np.arange(1, n * (n - 1) // 2 + 1)
        sq = distance.squareform(v)
        i, j = np.triu_indices(n, 1)
        assert np.array_equal(sq[i, j], v[edlib_amd.condensed_index(n, i, j)])
        assert np.array_equal(sq[j, i], v[edlib_amd.condensed_index(n, j, i)])


def _brute_nearest(n, first, second, ed):
    out = {f: np.full(n, -1, dtype=np.int32) for f in ("nearest", "nearestDistance", "secondDistance")}
    for s in range(n):
        keys = sorted((d, b if a == s else a) for a, b, d in zip(first, second, ed) if d >= 0 and s in (a, b))
        if keys:
            out["nearestDistance"][s], out["nearest"][s] = keys[0]
        if len(keys) > 1:
            out["secondDistance"][s] = keys[1][0]
    return out


def test_self_nearest_model_hand_made():
    # 0: partners 1 and 3 tie at 2 -> the lower index, second equals the best
    # 2: one partner within k (4, below and above mixed) -> second -1
    # 5: nothing within k
    # 4: best on the lower side (2, distance 1), second on the upper side (6, distance 3)
    first = [0, 0, 2, 4, 5, 1, 0]
    second = [1, 3, 4, 6, 6, 3, 5]
    ed = [2, 2, 1, 3, -1, 0, -1]
    got = edlib_amd.self_nearest_model(7, first, second, ed)
    assert got["nearest"].tolist() == [1, 3, 4, 1, 2, -1, 4]
    assert got["nearestDistance"].tolist() == [2, 0, 1, 0, 1, -1, 3]
    assert got["secondDistance"].tolist() == [2, 2, -1, 2, 3, -1, -1]
    want = _brute_nearest(7, first, second, ed)
    for f in want:
        assert np.array_equal(got[f], want[f]), f


@pytest.mark.parametrize("n", [0, 1, 2, 9, 40])
def test_self_nearest_model_matches_brute_force(n):
    rng = np.random.default_rng(n)
    i, j = np.triu_indices(n, 1)
    for seed in range(3):
        ed = rng.integers(-1, 4, size=len(i))
        if seed == 2:
            ed[:] = -1
        flip = rng.random(len(i)) < 0.5                 # the orientation of a listed pair does not matter
        a, b = np.where(flip, j, i), np.where(flip, i, j)
        got = edlib_amd.self_nearest_model(n, a, b, ed)
        want = _brute_nearest(n, a.tolist(), b.tolist(), ed.tolist())
        for f in want:
            assert np.array_equal(got[f], want[f]), (f, n, seed)
            assert got[f].dtype == np.int32 and got[f].shape == (n,)


def test_counter_formulas():
    assert self_cells([]) == 0 and self_cells([7]) == 0
    assert self_cells([3, 4, 5]) == 3 * 4 + 3 * 5 + 4 * 5
    assert self_word_steps([24] * 5, -1) == 10 * 24
    assert self_word_steps([24] * 5, 0) == 10 * 24
    # rows are the shorter sequence: 33 bases are two words only against something at least as long
    assert self_word_steps([33, 10], -1) == 1 * 33
    assert self_word_steps([33, 40], -1) == 2 * 40
    assert self_word_steps([33, 40], 6) == 0 and self_word_steps([33, 40], 7) == 2 * 40
    # empty sequences and those above the kernel's envelope are not scanned by it
    assert self_word_steps([0, 20, 300, 20], -1) == 20
