"""CPU: the both-strand self surface (edlibAmdBatchCreateSelfBothStrands / CreateSelfHitsBothStrands / SelfStrands) is
declared, exported, bound and laid out as documented, and everything a self batch does not take -- HW, SHW, tasks other
than DISTANCE, k < 0 for the hit list, a negative count, descending offsets -- is refused before any device is looked
for, with the messages of the one-strand Creates (test_self_api.py).  Without a device Create fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("edlibAmdBatchCreateSelfBothStrands", "edlibAmdBatchCreateSelfHitsBothStrands", "edlibAmdBatchSelfStrands")
FIELDS = ["numSequences", "numPairs", "numHits", "pairStrand", "hitStrand", "nearestStrand"]


def test_header_declares_self_strands_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in NAMES:
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    body = src[src.index("typedef struct {", src.index("edlibAmdBatchCreateSelfHitsBothStrands(")):src.index("EdlibAmdSelfStrands;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    # the complement condition is part of the contract
    assert "Eq(c(x), y) <=> Eq(x, c(y))" in src


def test_self_strands_symbols_exported_and_bound():
    import edlib_amd
    L = edlib_amd.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    assert L.edlibAmdBatchCreateSelfBothStrands.restype is C.c_void_p
    assert L.edlibAmdBatchCreateSelfHitsBothStrands.restype is C.c_void_p
    assert L.edlibAmdBatchCreateSelfBothStrands.argtypes == L.edlibAmdBatchCreateSelf.argtypes


def test_self_strands_struct_layout():
    import edlib_amd
    S = edlib_amd.SelfStrands
    assert [f for f, _ in S._fields_] == FIELDS
    assert C.sizeof(S) == 24 + 3 * 8
    assert S.numSequences.offset == 0 and S.numPairs.offset == 8 and S.numHits.offset == 16
    assert S.numPairs.size == 8 and S.numHits.size == 8
    for i, n in enumerate(FIELDS[3:]):
        assert getattr(S, n).offset == 24 + 8 * i, n


def _create(mode="NW", task="distance", k=-1, hits=False, n=2, offsets=(0, 4, 8)):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    s = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    o = np.array(offsets, dtype=np.int64)
    create = L.edlibAmdBatchCreateSelfHitsBothStrands if hits else L.edlibAmdBatchCreateSelfBothStrands
    h = create(s.ctypes.data, o.ctypes.data, n, cfg, 0)
    err = edlib_amd.last_error()
    if h:
        L.edlibAmdBatchDestroy(h)
    return h, err


@pytest.mark.parametrize("hits", [False, True])
@pytest.mark.parametrize("mode", ["HW", "SHW"])
def test_self_strands_refuse_other_modes(mode, hits):
    h, err = _create(mode=mode, k=1, hits=hits)
    assert not h
    assert "EDLIB_MODE_NW" in err and mode in err and "cross batch" in err


@pytest.mark.parametrize("hits", [False, True])
@pytest.mark.parametrize("task", ["locations", "path"])
def test_self_strands_refuse_other_tasks(task, hits):
    h, err = _create(task=task, k=1, hits=hits)
    assert not h
    assert "self batches compute distances only (EDLIB_TASK_DISTANCE)" in err


@pytest.mark.parametrize("k", [-1, -7])
def test_self_strands_hits_refuse_negative_k(k):
    h, err = _create(k=k, hits=True)
    assert not h
    assert "hit-list self batches need config.k >= 0" in err and "edlibAmdBatchCreateSelf" in err


@pytest.mark.parametrize("hits", [False, True])
def test_self_strands_refuse_bad_shapes(hits):
    h, err = _create(k=1, hits=hits, n=-1)
    assert not h and "bad batch shape" in err
    h, err = _create(k=1, hits=hits, offsets=(0, 6, 4))
    assert not h and "bad sequence offsets" in err
    import edlib_amd
    cfg, _ = edlib_amd._make_config("NW", "distance", 1, None)
    L = edlib_amd.lib()
    create = L.edlibAmdBatchCreateSelfHitsBothStrands if hits else L.edlibAmdBatchCreateSelfBothStrands
    assert not create(None, None, 3, cfg, 0)                       # sequences without offsets
    assert "bad batch shape" in edlib_amd.last_error()
    # more sequences than 2 n + 1 pool entries can index: refused on the count alone, before an offset is read
    o = np.zeros(1, dtype=np.int64)
    assert not create(None, o.ctypes.data, 0x40000000, cfg, 0)
    assert "bad both-strand batch shape" in edlib_amd.last_error()


def test_self_strands_python_refusals():
    import edlib_amd
    with pytest.raises(ValueError, match="strands"):
        edlib_amd.SelfBatch([b"ACGT", b"ACGA"], strands="sideways")
    with pytest.raises(ValueError, match="strands"):
        edlib_amd.pdist([b"ACGT", b"ACGA"], strands="sideways")
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.SelfBatch([b"ACGT", b"ACGA"], hits=True, strands="both")
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.pairs_within([b"ACGT", b"ACGA"], -1, strands="both")


def test_self_strands_view_refuses_null():
    import edlib_amd
    L = edlib_amd.lib()
    assert L.edlibAmdBatchSelfStrands(None, 3, C.byref(edlib_amd.SelfStrands())) != 0
    assert "null" in edlib_amd.last_error()


def test_self_strands_without_device_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.SelfBatch([b"ACGT", b"ACGA"], k=1, device=999, strands="both")
        return
    for hits in (False, True):
        h, err = _create(k=1, hits=hits)
        assert not h
        assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.pdist([b"ACGT", b"ACGA"], strands="both")
