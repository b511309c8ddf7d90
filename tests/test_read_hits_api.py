"""CPU: the hit-list read surface (edlibAmdBatchCreateSharedHits / edlibAmdBatchSharedHits) is declared, exported and laid
out as documented; what the batch does not take (k < 0, SHW / NW, LOC / PATH, reads above 256 bases, more than 16 target
symbols) is refused before any device is looked for, with the limit named; the Python guards raise; without a device Create
fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_read_hits_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in ("edlibAmdBatchCreateSharedHits", "edlibAmdBatchSharedHits"):
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    assert "EdlibAmdReadHits;" in src
    body = src[src.index("typedef struct {", src.index("edlibAmdBatchCreateSharedHits")):src.index("EdlibAmdReadHits;")]
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == ["numUnits", "numHits", "unitOffsets", "firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations"]


def test_read_hits_symbols_exported():
    import edlib_amd
    L = edlib_amd.lib()
    assert hasattr(L, "edlibAmdBatchCreateSharedHits") and hasattr(L, "edlibAmdBatchSharedHits")


def test_read_hits_layout():
    import edlib_amd
    H = edlib_amd.ReadHits
    assert [f for f, _ in H._fields_] == ["numUnits", "numHits", "unitOffsets", "firstEnd", "lastEnd", "editDistance",
                                          "endLocation", "numLocations"]
    assert C.sizeof(H) == 8 + 8 + 6 * 8
    assert H.numUnits.offset == 0 and H.numHits.offset == 8 and H.numHits.size == 8
    for i, n in enumerate(["unitOffsets", "firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations"]):
        assert getattr(H, n).offset == 16 + 8 * i, n


def _create(mode="HW", task="distance", k=2, reads=(b"ACGTACGT",), target=b"ACGTACGTAC"):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    qd, qo = edlib_amd._pack(list(reads))
    t = np.frombuffer(target, dtype=np.uint8)
    h = L.edlibAmdBatchCreateSharedHits(qd.ctypes.data, qo.ctypes.data, len(reads), t.ctypes.data, len(target), cfg, 0)
    return h, edlib_amd.last_error()


@pytest.mark.parametrize("what,kw,names", [
    ("k", dict(k=-1), "k must be >= 0"),
    ("shw", dict(mode="SHW"), "EDLIB_MODE_HW"),
    ("nw", dict(mode="NW"), "EDLIB_MODE_HW"),
    ("loc", dict(task="locations"), "EDLIB_TASK_DISTANCE"),
    ("path", dict(task="path"), "EDLIB_TASK_DISTANCE"),
    ("long", dict(reads=(b"ACGT", b"A" * 257)), "the limit is 256"),
    ("symbols", dict(target=bytes(range(65, 82))), "the limit is 16"),
])
def test_read_hits_refusals_name_the_limit(what, kw, names):
    h, err = _create(**kw)
    assert not h
    assert names in err, err
    if what == "long":
        assert "read 1" in err and "257" in err
    if what == "symbols":
        assert "17" in err


def test_read_hits_python_guards():
    import edlib_amd
    with pytest.raises(RuntimeError, match="k must be >= 0"):
        edlib_amd.SharedBatch([b"ACGT"], b"ACGTACGT", k=-1, hits=True)
    with pytest.raises(RuntimeError, match="EDLIB_MODE_HW"):
        edlib_amd.SharedBatch([b"ACGT"], b"ACGTACGT", mode="NW", k=1, hits=True)
    with pytest.raises(RuntimeError, match="k must be >= 0"):
        edlib_amd.find_all([b"ACGT"], b"ACGTACGT", -1)
    # the guards answer before the handle is looked at
    plain = edlib_amd.SharedBatch.__new__(edlib_amd.SharedBatch)
    plain._h, plain.n, plain.is_hits = None, 1, False
    with pytest.raises(RuntimeError, match="hits=True"):
        plain.hits()
    listing = edlib_amd.SharedBatch.__new__(edlib_amd.SharedBatch)
    listing._h, listing.n, listing.is_hits = None, 1, True
    for call in (listing.results, listing.results_flat, listing.cigars):
        with pytest.raises(RuntimeError, match="use hits\\(\\)"):
            call()


def test_read_hits_without_device_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.SharedBatch([b"ACGT"], b"ACGTACGT", k=1, device=999, hits=True)
        return
    h, err = _create()
    assert not h
    assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.SharedBatch([b"ACGT"], b"ACGTACGT", k=1, hits=True)
