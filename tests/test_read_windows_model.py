"""CPU: the window a read batch's first hit is re-aligned in (edlib_amd.first_hit_windows, DESIGN.md §4b "Pairs from a
read batch").  For a read of m bases with HW distance d and first end location e >= 0 the checker's whole-target HW / PATH
answer must equal its answer over target[max(0, e - m - d + 1) .. e], shifted by the window's start: the distance, the
first end, the first start and every op byte -- also where the window is padded on the left.  And first_hit_windows must
name exactly the reads that have such a hit: not those with nothing within k, not those whose first end is -1."""
import numpy as np
import pytest

import edlib_amd


def _cases(seed, count):
    """(read, target, k): targets of 50, 300 and 2,000 bases over 2 to 5 symbols; reads of 1 to 200 bases cut from the
    target at 0 to 30 % error, or unrelated; k in -1, 3, 10"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        T = (50, 300, 2000)[i % 3]
        sigma = int(rng.integers(2, 6))
        A = np.frombuffer(b"ACGTN", dtype=np.uint8)[:sigma]
        t = A[rng.integers(0, sigma, T)]
        m = int(rng.integers(1, min(200, T) + 1))
        if rng.random() < 0.2:
            q = A[rng.integers(0, sigma, m)]
        else:
            s = int(rng.integers(0, T - m + 1))
            q = t[s:s + m].copy()
            err = rng.random() * 0.3
            hit = rng.random(m) < err
            q[hit] = A[rng.integers(0, sigma, int(hit.sum()))]
            if m > 3 and rng.random() < 0.5:
                p = int(rng.integers(1, m - 1))
                q = np.concatenate([q[:p], q[p + 1:]]) if rng.random() < 0.5 else np.concatenate([q[:p], A[:1], q[p:]])
        out.append((q.tobytes(), t.tobytes(), (-1, 3, 10)[int(rng.integers(0, 3))]))
    return out


def _flat(results):
    """what results_flat() of a read batch holds of these results"""
    loc = np.zeros(len(results) + 1, dtype=np.int64)
    loc[1:] = np.cumsum([r["numLocations"] for r in results])
    ends = np.array([e for r in results for e in (r["endLocations"] or [])], dtype=np.int32)
    return {"editDistance": np.array([r["editDistance"] for r in results], dtype=np.int32), "locOff": loc, "ends": ends}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_first_hit_window_gives_the_whole_targets_path(checker, seed):
    cases = _cases(seed, 300)
    whole = [checker.align(q, t, "HW", "path", k) for q, t, k in cases]
    flat = _flat(whole)
    read, start, length, strand = edlib_amd.first_hit_windows(flat, [len(q) for q, _, _ in cases])
    assert strand is None and read.dtype == start.dtype == length.dtype == np.int32
    # exactly the reads with a hit whose first end is a column
    want = [i for i, r in enumerate(whole) if r["editDistance"] >= 0 and r["endLocations"][0] >= 0]
    assert read.tolist() == want
    left_out = set(range(len(cases))) - set(want)
    assert any(whole[i]["editDistance"] < 0 for i in left_out)
    several = 0
    for i, s, n in zip(read, start, length):
        q, t, k = cases[i]
        w = whole[i]
        d, e, m = w["editDistance"], w["endLocations"][0], len(q)
        assert s == max(0, e - m - d + 1) and n == e + 1 - s and n >= 1
        several += w["numLocations"] > 1
        for pad in (0, 7):                                   # the caller's own padding on the left changes nothing
            s2 = max(0, int(s) - pad)
            got = checker.align(q, t[s2:e + 1], "HW", "path", k)
            assert got["editDistance"] == d, (i, pad)
            assert got["endLocations"][0] + s2 == e, (i, pad)
            assert got["startLocations"][0] + s2 == w["startLocations"][0], (i, pad)
            assert got["alignment"] == w["alignment"], (i, pad)
    assert len(want) > 150 and several > 30


def test_reads_without_a_column_to_end_at_are_left_out():
    """hand-made results: nothing within k, a first end of -1 (the whole read against the empty prefix), a first hit at
    column 0, a hit whose window would start before column 0; with the strands of a both-strand batch"""
    flat = {"editDistance": np.array([-1, 4, 0, 2, 5], dtype=np.int32),
            "locOff": np.array([0, 0, 2, 3, 5, 6], dtype=np.int64),
            "ends": np.array([-1, 9, 0, 3, 40, 199], dtype=np.int32)}
    m = [30, 4, 1, 10, 50]
    st = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    read, start, length, strand = edlib_amd.first_hit_windows(flat, m, st)
    assert read.tolist() == [2, 3, 4]
    assert start.tolist() == [0, 0, 199 - 50 - 5 + 1]
    assert length.tolist() == [1, 4, 55]
    assert strand.dtype == np.uint8 and strand.tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        edlib_amd.first_hit_windows(flat, m[:-1])
