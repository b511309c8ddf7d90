"""CPU: the neighbours surface of self and cross batches (edlibAmdBatchSelfNeighbors, edlibAmdBatchCrossNeighbors) is
declared, exported, bound and laid out as documented, and what it refuses without looking at a device -- K out of range, a
NULL batch, a NULL out -- is refused with its message.  The Python entry points exist and refuse what the Creates refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["numRows", "K", "count", "neighbor", "distance", "strand"]
CALLS = ["edlibAmdBatchSelfNeighbors", "edlibAmdBatchCrossNeighbors"]


def test_header_declares_neighbors_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for fn in CALLS:
        assert re.search(r"EDLIB_API\s+int\s+" + fn + r"\s*\(\s*EdlibAmdBatch\*\s*batch,\s*int\s+K,\s*int\s+maxDistance,"
                         r"\s*EdlibAmdNeighbors\*\s*out\)", src), fn
    end = src.index("} EdlibAmdNeighbors;")
    body = re.sub(r"/\*.*?\*/", "", src[src.rindex("typedef struct {", 0, end):end], flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    assert "(distance << 32) | index" in src                         # the order is part of the contract
    assert "K is 1..64" in src


def test_neighbors_symbols_exported_and_bound():
    import edlib_amd
    L = edlib_amd.lib()
    for fn in CALLS:
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes[1:3] == [C.c_int, C.c_int]
    for f in ("knn", "neighbors_model"):
        assert callable(getattr(edlib_amd, f))
    assert callable(edlib_amd.SelfBatch.neighbors) and callable(edlib_amd.CrossBatch.neighbors)


def test_neighbors_struct_layout():
    import edlib_amd
    S = edlib_amd.Neighbors
    assert [f for f, _ in S._fields_] == FIELDS
    assert C.sizeof(S) == 8 + 4 * 8
    assert S.numRows.offset == 0 and S.K.offset == 4
    for i, n in enumerate(FIELDS[2:]):
        assert getattr(S, n).offset == 8 + 8 * i, n
    assert S._fields_[5][1] == C.POINTER(C.c_ubyte)


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("K", [0, -1, 65, 1 << 20])
def test_neighbors_refuse_k_out_of_range(fn, K):
    import edlib_amd
    L = edlib_amd.lib()
    out = edlib_amd.Neighbors()
    assert getattr(L, fn)(None, K, -1, C.byref(out)) != 0
    err = edlib_amd.last_error()
    assert fn in err and "K must be 1..64 (got %d)" % K in err


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("K", [1, 64])
def test_neighbors_refuse_null(fn, K):
    import edlib_amd
    L = edlib_amd.lib()
    assert getattr(L, fn)(None, K, -1, C.byref(edlib_amd.Neighbors())) != 0
    assert fn in edlib_amd.last_error() and "null" in edlib_amd.last_error()
    assert getattr(L, fn)(None, K, 0, None) != 0
    assert "null" in edlib_amd.last_error()


def test_knn_python_refusals():
    import edlib_amd
    with pytest.raises(ValueError, match="strands"):
        edlib_amd.knn([b"ACGT", b"ACGA"], 1, strands="sideways")


def test_neighbors_model_shapes():
    import edlib_amd
    got = edlib_amd.neighbors_model(3, [0, 1, 1, 2], [1, 0, 2, 1], [2, 2, 1, 1], 2, -1)
    assert got["count"].tolist() == [1, 2, 1]
    assert got["neighbor"].tolist() == [[1, -1], [2, 0], [1, -1]]
    assert got["distance"].tolist() == [[2, -1], [1, 2], [1, -1]]
    assert all(got[f].dtype == np.int32 for f in got)
