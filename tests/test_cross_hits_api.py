"""CPU: the hit-list cross surface (edlibAmdBatchCreateCrossHits / edlibAmdBatchCrossHits) is declared, exported and laid
out as documented; k < 0 and tasks other than DISTANCE are refused before any device is looked for, and without a device
Create fails loudly.  hits_model() / best_from_hits() are the host statement of the CSR layout and of the best hits reduced
from a list; they are checked here against best_model() of the dense matrix."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_cross_api import best_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hits_model(ed, nloc=None, end=None):
    """The hit list of a dense (numTargets, numQueries) matrix: the cells whose editDistance is not -1, grouped by target,
    ascending query inside a target.  Returns targetOffsets [nt + 1] and query / editDistance (/ numLocations /
    endLocation) [numHits]."""
    nt, nq = ed.shape
    t, q = np.nonzero(ed != -1)                     # row-major: target-major, ascending query
    off = np.zeros(nt + 1, dtype=np.int64)
    np.cumsum(np.bincount(t, minlength=nt), out=off[1:])
    out = {"targetOffsets": off, "query": q.astype(np.int32), "editDistance": ed[t, q].astype(np.int32)}
    if nloc is not None:
        out["numLocations"] = nloc[t, q].astype(np.int32)
    if end is not None:
        out["endLocation"] = end[t, q].astype(np.int32)
    return out


def best_from_hits(h, nq):
    """Best hits from a CSR list, as the device reduces them: per target over its queries and per query over its targets,
    pass 1 the smallest (distance << 32 | index) key, pass 2 the smallest key other than it."""
    off = h["targetOffsets"]
    nt = len(off) - 1
    t = np.repeat(np.arange(nt, dtype=np.int64), np.diff(off))
    q = h["query"].astype(np.int64)
    d = h["editDistance"].astype(np.int64)
    none = np.iinfo(np.uint64).max

    def reduce(owner, idx, n):
        key = ((d << 32) | idx).astype(np.uint64)
        b1 = np.full(n, none, dtype=np.uint64)
        np.minimum.at(b1, owner, key)
        b2 = np.full(n, none, dtype=np.uint64)
        other = key != b1[owner]
        np.minimum.at(b2, owner[other], key[other])
        bi = np.where(b1 == none, -1, (b1 & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
        bd = np.where(b1 == none, -1, (b1 >> np.uint64(32)).astype(np.int64)).astype(np.int32)
        sd = np.where(b2 == none, -1, (b2 >> np.uint64(32)).astype(np.int64)).astype(np.int32)
        return bi, bd, sd
    bq, bqd, sqd = reduce(t, q, nt)
    bt, btd, std = reduce(q, t, nq)
    return {"bestQuery": bq, "bestQueryDistance": bqd, "secondQueryDistance": sqd,
            "bestTarget": bt, "bestTargetDistance": btd, "secondTargetDistance": std}


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (7, 64), (40, 9), (0, 4), (4, 0), (33, 17)])
def test_best_from_hits_matches_dense_model(shape):
    for seed in range(4):
        rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + seed)
        ed = rng.integers(-1, 4, size=shape).astype(np.int32)          # many ties and -1 cells
        if shape[0] > 2 and shape[1] > 0:
            ed[1, :] = -1
            ed[2, :] = 2
        if shape[1] > 1 and shape[0] > 0:
            ed[:, 0] = -1
        if seed == 3:
            ed[:] = -1                                                   # no hits at all
        h = hits_model(ed)
        assert h["targetOffsets"][-1] == np.count_nonzero(ed != -1)
        for t in range(shape[0]):                                        # CSR: each target's queries, ascending
            s, e = h["targetOffsets"][t], h["targetOffsets"][t + 1]
            assert np.array_equal(h["query"][s:e], np.nonzero(ed[t] != -1)[0])
            assert np.array_equal(h["editDistance"][s:e], ed[t][ed[t] != -1])
        got = best_from_hits(h, shape[1])
        want = best_model(ed)
        for f in want:
            assert np.array_equal(got[f], want[f]), (f, shape, seed)


def test_header_declares_cross_hits_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in ("edlibAmdBatchCreateCrossHits", "edlibAmdBatchCrossHits"):
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    assert "EdlibAmdCrossHits;" in src
    body = src[src.index("typedef struct {", src.index("edlibAmdBatchCreateCrossHits")):src.index("EdlibAmdCrossHits;")]
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == ["numTargets", "numHits", "targetOffsets", "query", "editDistance", "numLocations", "endLocation"]


def test_cross_hits_symbols_exported():
    import edlib_amd
    L = edlib_amd.lib()
    assert hasattr(L, "edlibAmdBatchCreateCrossHits") and hasattr(L, "edlibAmdBatchCrossHits")


def test_cross_hits_layout():
    import edlib_amd
    H = edlib_amd.CrossHits
    assert C.sizeof(H) == 8 + 8 + 5 * 8
    assert H.numQueries.offset == 0 and H.numTargets.offset == 4 and H.numHits.offset == 8
    for i, n in enumerate(["targetOffsets", "query", "editDistance", "numLocations", "endLocation"]):
        assert getattr(H, n).offset == 16 + 8 * i, n
    assert H.numHits.size == 8 and H.targetOffsets.size == 8


def _create(task, k, mode="NW"):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    q = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    o = np.array([0, 4, 8], dtype=np.int64)
    h = L.edlibAmdBatchCreateCrossHits(q.ctypes.data, o.ctypes.data, 2, q.ctypes.data, o.ctypes.data, 2, cfg, 0)
    return h, edlib_amd.last_error()


@pytest.mark.parametrize("k", [-1, -5])
def test_cross_hits_refuses_negative_k(k):
    h, err = _create("distance", k)
    assert not h
    assert "k >= 0" in err


@pytest.mark.parametrize("task", ["locations", "path"])
def test_cross_hits_refuses_other_tasks(task):
    h, err = _create(task, 2)
    assert not h
    assert "DISTANCE" in err


def test_cross_hits_python_refuses_negative_k():
    import edlib_amd
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], mode="NW", k=-1, hits=True)
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.align_cross([b"ACGT"], [b"ACGT"], mode="HW", hits=True)


def test_cross_hits_without_device_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], k=1, device=999, hits=True)
        return
    h, err = _create("distance", 1)
    assert not h
    assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], k=1, hits=True)
