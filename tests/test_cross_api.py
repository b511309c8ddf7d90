"""CPU: the cross-batch surface (edlibAmdBatchCreateCross / edlibAmdBatchCrossView) is declared, exported and laid out
as documented; without a device Create fails loudly, and a task other than DISTANCE is refused.  best_model() is the
host statement of the best-hit rules the GPU tests reduce the matrix with; it is checked here against a brute force."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def best_model(ed):
    """ed: (numTargets, numQueries) distances, -1 = not within k.  Per target over the queries and per query over the
    targets: best index (ties: lowest), best distance, smallest distance over the other indices; -1 where none."""
    def rows(a):
        n, w = a.shape
        key = np.where(a >= 0, a.astype(np.int64) * (1 << 32) + np.arange(w, dtype=np.int64)[None, :], np.iinfo(np.int64).max)
        order = np.sort(key, axis=1) if w else np.zeros((n, 0), dtype=np.int64)
        none = np.iinfo(np.int64).max

        def split(col):
            k = order[:, col] if w > col else np.full(n, none)
            return np.where(k == none, -1, k & 0xffffffff).astype(np.int32), np.where(k == none, -1, k >> 32).astype(np.int32)
        bi, bd = split(0)
        _, sd = split(1)
        return bi, bd, sd
    bq, bqd, sqd = rows(ed)
    bt, btd, std = rows(ed.T)
    return {"bestQuery": bq, "bestQueryDistance": bqd, "secondQueryDistance": sqd,
            "bestTarget": bt, "bestTargetDistance": btd, "secondTargetDistance": std}


def _brute(ed):
    def one(row):
        live = [(d, i) for i, d in enumerate(row) if d >= 0]
        if not live:
            return -1, -1, -1
        d, i = min(live)
        others = [x for x, j in live if j != i]
        return i, d, (min(others) if others else -1)
    out = {}
    r = [one(ed[t]) for t in range(ed.shape[0])]
    c = [one(ed[:, q]) for q in range(ed.shape[1])]
    for n, (a, b) in (("Query", (r, 0)), ("Target", (c, 0))):
        out["best" + n] = np.array([x[0] for x in a], dtype=np.int32)
        out["best" + n + "Distance"] = np.array([x[1] for x in a], dtype=np.int32)
        out["second" + n + "Distance"] = np.array([x[2] for x in a], dtype=np.int32)
    return out


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (7, 64), (40, 9), (0, 4), (4, 0)])
def test_best_model_matches_brute_force(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    ed = rng.integers(-1, 4, size=shape).astype(np.int32)          # many ties and -1 cells
    if shape[0] > 2 and shape[1] > 0:
        ed[1, :] = -1                                              # a row with nothing within k
        ed[2, :] = 2                                               # a row of one distance
    if shape[1] > 1 and shape[0] > 0:
        ed[:, 0] = -1
    want = _brute(ed)
    got = best_model(ed)
    for f in want:
        assert np.array_equal(got[f], want[f]), f


def test_header_declares_cross_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in ("edlibAmdBatchCreateCross", "edlibAmdBatchCrossView"):
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    assert "EdlibAmdCrossView;" in src
    assert re.search(r"#define\s+EDLIB_AMD_CROSS_MATRIX\s+1\b", src)
    assert re.search(r"#define\s+EDLIB_AMD_CROSS_BEST\s+2\b", src)


def test_cross_symbols_exported():
    import edlib_amd
    L = edlib_amd.lib()
    assert hasattr(L, "edlibAmdBatchCreateCross") and hasattr(L, "edlibAmdBatchCrossView")


def test_cross_view_layout():
    import edlib_amd
    V = edlib_amd.CrossView
    assert C.sizeof(V) == 8 + 9 * 8
    assert V.numQueries.offset == 0 and V.numTargets.offset == 4
    names = ["editDistance", "numLocations", "endLocation", "bestQuery", "bestQueryDistance", "secondQueryDistance",
             "bestTarget", "bestTargetDistance", "secondTargetDistance"]
    for i, n in enumerate(names):
        assert getattr(V, n).offset == 8 + 8 * i, n
    assert edlib_amd.CROSS_MATRIX == 1 and edlib_amd.CROSS_BEST == 2


def _create(task):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config("HW", task, -1, None)
    q = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    o = np.array([0, 4, 8], dtype=np.int64)
    h = L.edlibAmdBatchCreateCross(q.ctypes.data, o.ctypes.data, 2, q.ctypes.data, o.ctypes.data, 2, cfg, 0)
    return h, edlib_amd.last_error()


@pytest.mark.parametrize("task", ["locations", "path"])
def test_cross_refuses_other_tasks(task):
    h, err = _create(task)
    assert not h
    assert "DISTANCE" in err


def test_cross_without_device_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], device=999)
        return
    h, err = _create("distance")
    assert not h
    assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"])
