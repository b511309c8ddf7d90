"""CPU: the window a best cell of a cross batch is re-aligned in (edlib_amd.cell_windows, DESIGN.md §4b "Pairs from a
cross batch").  For a cell of a query of m bases with distance d and first end location e the checker's whole-target
PATH answer must equal its answer over the window cell_windows names -- HW: target[max(0, e - m - d + 1) .. e], SHW:
target[0 .. e], NW: the whole target --, shifted by the window's start: the distance, the first end, the first start and
every op byte; for HW also where the caller pads the window on the left.  And cell_windows must keep exactly the cells
that have such a window: not those with nothing within k, not those whose first end is -1, not those of an empty
target."""
import numpy as np
import pytest

import edlib_amd

MODES = ("HW", "SHW", "NW")


def _cases(seed, count, mode):
    """queries, targets and the cells (query, target, k) between them: targets of 0, 50, 300 and 2,000 bases over 2 to 5
    symbols; queries of 1 to 200 bases cut from a target at 0 to 30 % error (NW: about the target's length), or
    unrelated; k in -1, 3, 10"""
    rng = np.random.default_rng(seed)
    A = np.frombuffer(b"ACGTN", dtype=np.uint8)
    queries, targets, cells = [], [b""], []
    for i in range(count):
        T = (50, 300, 2000)[i % 3]
        sigma = int(rng.integers(2, 6))
        t = A[rng.integers(0, sigma, T)]
        m = int(rng.integers(1, min(200, T) + 1))
        if rng.random() < 0.2:
            q = A[rng.integers(0, sigma, m)]
        else:
            if mode == "NW":
                T = m + int(rng.integers(0, 4))
                t = t[:T]
            s = 0 if mode != "HW" else int(rng.integers(0, T - m + 1))
            q = t[s:s + m].copy()
            hit = rng.random(m) < rng.random() * 0.3
            q[hit] = A[rng.integers(0, sigma, int(hit.sum()))]
            if m > 3 and rng.random() < 0.5:
                p = int(rng.integers(1, m - 1))
                q = np.concatenate([q[:p], q[p + 1:]]) if rng.random() < 0.5 else np.concatenate([q[:p], A[:1], q[p:]])
        queries.append(q.tobytes())
        targets.append(t.tobytes())
        cells.append((i, i + 1, (-1, 3, 10)[int(rng.integers(0, 3))]))
        if i % 25 == 0:
            cells.append((i, 0, -1))                         # the empty target
    return queries, targets, cells


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [1, 2])
def test_the_cell_window_gives_the_whole_targets_path(checker, mode, seed):
    queries, targets, cells = _cases(seed, 300, mode)
    whole = [checker.align(queries[q], targets[t], mode, "path", k) for q, t, k in cells]
    ed = [w["editDistance"] for w in whole]
    end = [w["endLocations"][0] if w["editDistance"] >= 0 and w["endLocations"] else -1 for w in whole]
    kept, pq, pt, ps, pl, st = edlib_amd.cell_windows(mode, [c[0] for c in cells], [c[1] for c in cells], ed, end,
                                                      [len(q) for q in queries], [len(t) for t in targets])
    assert st is None and kept.dtype == np.int64 and pq.dtype == pt.dtype == ps.dtype == pl.dtype == np.int32
    # exactly the cells within k whose first end is a column of a target that has one
    want = [i for i, (c, w) in enumerate(zip(cells, whole))
            if w["editDistance"] >= 0 and len(targets[c[1]]) > 0 and (mode == "NW" or end[i] >= 0)]
    assert kept.tolist() == want
    left_out = set(range(len(cells))) - set(want)
    assert any(ed[i] < 0 for i in left_out) and any(cells[i][1] == 0 for i in left_out)
    several = 0
    for i, q, t, s, n in zip(kept, pq, pt, ps, pl):
        assert (q, t) == cells[i][:2]
        w, k = whole[i], cells[i][2]
        d, e, m, T = w["editDistance"], w["endLocations"][0], len(queries[q]), len(targets[t])
        if mode == "HW":
            assert s == max(0, e - m - d + 1) and n == e + 1 - s
        elif mode == "SHW":
            assert s == 0 and n == e + 1
        else:
            assert s == 0 and n == T == e + 1
        assert n >= 1 and s + n <= T
        several += w["numLocations"] > 1
        for pad in ((0, 7) if mode == "HW" else (0,)):      # the caller's own padding on the left changes nothing
            s2 = max(0, int(s) - pad)
            got = checker.align(queries[q], targets[t][s2:int(s) + int(n)], mode, "path", k)
            assert got["editDistance"] == d, (i, pad)
            assert got["endLocations"][0] + s2 == e, (i, pad)
            assert got["startLocations"][0] + s2 == w["startLocations"][0], (i, pad)
            assert got["alignment"] == w["alignment"], (i, pad)
    assert len(want) > 150 and (mode == "NW" or several > 20)


def test_cells_without_a_window_are_left_out():
    """hand-made cells: nothing within k, a first end of -1 (the whole query against the empty prefix), an empty target,
    a hit at column 0, a hit whose HW window would start before column 0; with the strand bytes of a both-strand batch"""
    ql, tl = [30, 4, 1, 10, 50], [0, 200, 12]
    q = [0, 1, 2, 3, 4, 2]
    t = [1, 1, 1, 2, 1, 0]
    d = np.array([-1, 4, 0, 2, 5, 1], dtype=np.int32)
    e = np.array([-1, -1, 0, 3, 199, -1], dtype=np.int32)
    st = np.array([0, 1, 3, 0, 1, 1], dtype=np.uint8)       # (bit 1: the other strand ties -- not the pair's strand)
    kept, pq, pt, ps, pl, strand = edlib_amd.cell_windows("HW", q, t, d, e, ql, tl, st)
    assert kept.tolist() == [2, 3, 4] and pq.tolist() == [2, 3, 4] and pt.tolist() == [1, 2, 1]
    assert ps.tolist() == [0, 0, 199 - 50 - 5 + 1] and pl.tolist() == [1, 4, 55]
    assert strand.dtype == np.uint8 and strand.tolist() == [1, 0, 1]
    kept, pq, pt, ps, pl, strand = edlib_amd.cell_windows("SHW", q, t, d, e, ql, tl)
    assert kept.tolist() == [2, 3, 4] and ps.tolist() == [0, 0, 0] and pl.tolist() == [1, 4, 200] and strand is None
    e_nw = np.array([-1, 199, 199, 11, 199, -1], dtype=np.int32)
    kept, pq, pt, ps, pl, strand = edlib_amd.cell_windows("NW", q, t, d, e_nw, ql, tl)
    assert kept.tolist() == [1, 2, 3, 4] and ps.tolist() == [0] * 4 and pl.tolist() == [200, 200, 12, 200]
    with pytest.raises(ValueError):
        edlib_amd.cell_windows("HW", q, t, d, e[:-1], ql, tl)
    with pytest.raises(ValueError):
        edlib_amd.cell_windows("XX", q, t, d, e, ql, tl)
