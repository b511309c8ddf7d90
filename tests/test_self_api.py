"""CPU: the self-batch surface (edlibAmdBatchCreateSelf / CreateSelfHits / SelfView / SelfHits) is declared, exported and
laid out as documented, and everything a self batch does not take -- HW, SHW, tasks other than DISTANCE, k < 0 for the
hit list, a negative count, descending offsets -- is refused before any device is looked for, with the reason in
edlibAmdLastError().  Without a device Create fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("edlibAmdBatchCreateSelf", "edlibAmdBatchCreateSelfHits", "edlibAmdBatchSelfView", "edlibAmdBatchSelfHits")


def test_header_declares_self_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in NAMES:
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    body = src[src.index("typedef struct {", src.index("edlibAmdBatchCreateSelfHits(")):src.index("EdlibAmdSelfView;")]
    assert re.findall(r"\b(\w+)\s*;", body) == ["numSequences", "numPairs", "editDistance", "nearest", "nearestDistance",
                                                 "secondDistance"]
    body = src[src.index("typedef struct {", src.index("EdlibAmdSelfView;")):src.index("EdlibAmdSelfHits;")]
    assert re.findall(r"\b(\w+)\s*;", body) == ["numSequences", "numHits", "rowOffsets", "partner", "editDistance"]
    assert re.search(r"#define\s+EDLIB_AMD_SELF_DISTANCES\s+1\b", src) and re.search(r"#define\s+EDLIB_AMD_SELF_NEAREST\s+2\b", src)


def test_self_symbols_exported_and_bound():
    import edlib_amd
    L = edlib_amd.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    assert L.edlibAmdBatchCreateSelf.restype is C.c_void_p and L.edlibAmdBatchCreateSelfHits.restype is C.c_void_p
    assert (edlib_amd.SELF_DISTANCES, edlib_amd.SELF_NEAREST) == (1, 2)


def test_self_struct_layouts():
    import edlib_amd
    V, H = edlib_amd.SelfView, edlib_amd.SelfHits
    assert C.sizeof(V) == 16 + 4 * 8
    assert V.numSequences.offset == 0 and V.numPairs.offset == 8 and V.numPairs.size == 8
    for i, n in enumerate(["editDistance", "nearest", "nearestDistance", "secondDistance"]):
        assert getattr(V, n).offset == 16 + 8 * i, n
    assert C.sizeof(H) == 16 + 3 * 8
    assert H.numSequences.offset == 0 and H.numHits.offset == 8 and H.numHits.size == 8
    for i, n in enumerate(["rowOffsets", "partner", "editDistance"]):
        assert getattr(H, n).offset == 16 + 8 * i, n


def _create(mode="NW", task="distance", k=-1, hits=False, n=2, offsets=(0, 4, 8)):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    s = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    o = np.array(offsets, dtype=np.int64)
    create = L.edlibAmdBatchCreateSelfHits if hits else L.edlibAmdBatchCreateSelf
    h = create(s.ctypes.data, o.ctypes.data, n, cfg, 0)
    err = edlib_amd.last_error()
    if h:
        L.edlibAmdBatchDestroy(h)
    return h, err


@pytest.mark.parametrize("hits", [False, True])
@pytest.mark.parametrize("mode", ["HW", "SHW"])
def test_self_refuses_other_modes(mode, hits):
    h, err = _create(mode=mode, k=1, hits=hits)
    assert not h
    assert "EDLIB_MODE_NW" in err and mode in err and "cross batch" in err


@pytest.mark.parametrize("hits", [False, True])
@pytest.mark.parametrize("task", ["locations", "path"])
def test_self_refuses_other_tasks(task, hits):
    h, err = _create(task=task, k=1, hits=hits)
    assert not h
    assert "self batches compute distances only (EDLIB_TASK_DISTANCE)" in err


@pytest.mark.parametrize("k", [-1, -7])
def test_self_hits_refuse_negative_k(k):
    h, err = _create(k=k, hits=True)
    assert not h
    assert "hit-list self batches need config.k >= 0" in err and "edlibAmdBatchCreateSelf" in err


@pytest.mark.parametrize("hits", [False, True])
def test_self_refuses_bad_shapes(hits):
    h, err = _create(k=1, hits=hits, n=-1)
    assert not h and "bad batch shape" in err
    h, err = _create(k=1, hits=hits, offsets=(0, 6, 4))
    assert not h and "bad sequence offsets" in err
    import edlib_amd
    cfg, _ = edlib_amd._make_config("NW", "distance", 1, None)
    L = edlib_amd.lib()
    create = L.edlibAmdBatchCreateSelfHits if hits else L.edlibAmdBatchCreateSelf
    assert not create(None, None, 3, cfg, 0)                       # sequences without offsets
    assert "bad batch shape" in edlib_amd.last_error()


def test_self_python_refusals():
    import edlib_amd
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.SelfBatch([b"ACGT", b"ACGA"], hits=True)
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.pairs_within([b"ACGT", b"ACGA"], -1)


def test_self_views_refuse_null_and_other_batches():
    import edlib_amd
    L = edlib_amd.lib()
    assert L.edlibAmdBatchSelfView(None, 1, C.byref(edlib_amd.SelfView())) != 0
    assert L.edlibAmdBatchSelfHits(None, C.byref(edlib_amd.SelfHits())) != 0


def test_self_without_device_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.SelfBatch([b"ACGT", b"ACGA"], k=1, device=999)
        return
    for hits in (False, True):
        h, err = _create(k=1, hits=hits)
        assert not h
        assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.pdist([b"ACGT", b"ACGA"])
