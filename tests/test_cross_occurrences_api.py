"""CPU: the occurrence cross surface (edlibAmdBatchCreateCrossOccurrences / edlibAmdBatchCrossOccurrences) is declared,
exported and laid out as documented; what the batch does not take (NW / SHW, LOC / PATH, k < 0, a query above 256 bases, a
target with more than 16 symbols of its own, a bad shape) is refused before any device is looked for, with the limit named;
the Python argument checks raise before the library is called; without a device Create fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("edlibAmdBatchCreateCrossOccurrences", "edlibAmdBatchCrossOccurrences")
FIELDS = ["numTargets", "numHits", "targetOffsets", "query", "firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations"]


def test_header_declares_cross_occurrences_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in NAMES:
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    assert "EdlibAmdCrossOccurrences;" in src
    body = src[src.index("typedef struct {", src.index("edlibAmdBatchCreateCrossOccurrences(")):src.index("EdlibAmdCrossOccurrences;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    assert "numQueries, numTargets;" in body


def test_cross_occurrences_symbols_exported():
    import edlib_amd
    L = edlib_amd.lib()
    for n in NAMES:
        assert hasattr(L, n), n


def test_cross_occurrences_layout():
    import edlib_amd
    H = edlib_amd.CrossOccurrences
    assert [f for f, _ in H._fields_] == ["numQueries"] + FIELDS
    assert C.sizeof(H) == 8 + 8 + 7 * 8
    assert H.numQueries.offset == 0 and H.numTargets.offset == 4 and H.numHits.offset == 8 and H.numHits.size == 8
    for i, n in enumerate(FIELDS[2:]):
        assert getattr(H, n).offset == 16 + 8 * i, n


def _create(mode="HW", task="distance", k=2, queries=(b"ACGT", b"ACGTACGT"), targets=(b"ACGTACGTAC", b"TTTT"), nq=None,
            nt=None, qoff=None, toff=None):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    qd, qo = edlib_amd._pack(list(queries))
    td, to = edlib_amd._pack(list(targets))
    if qoff is not None:
        qo = np.asarray(qoff, dtype=np.int64)
    if toff is not None:
        to = np.asarray(toff, dtype=np.int64)
    h = L.edlibAmdBatchCreateCrossOccurrences(qd.ctypes.data, qo.ctypes.data, len(queries) if nq is None else nq,
                                              td.ctypes.data, to.ctypes.data, len(targets) if nt is None else nt, cfg, 0)
    return h, edlib_amd.last_error()


@pytest.mark.parametrize("what,kw,names", [
    ("nw", dict(mode="NW"), "EDLIB_MODE_HW"),
    ("shw", dict(mode="SHW"), "EDLIB_MODE_HW"),
    ("loc", dict(task="locations"), "EDLIB_TASK_DISTANCE"),
    ("path", dict(task="path"), "EDLIB_TASK_DISTANCE"),
    ("k", dict(k=-1), "k must be >= 0"),
    ("long", dict(queries=(b"ACGT", b"A" * 257)), "the limit is 256"),
    ("symbols", dict(targets=(b"ACGT", bytes(range(65, 82)))), "the limit is 16"),
    ("shape", dict(nq=-1), "bad batch shape"),
    ("shape", dict(nt=-2), "bad batch shape"),
    ("offsets", dict(qoff=[0, 8, 4]), "bad query offsets"),
    ("offsets", dict(toff=[0, 10, 3]), "bad target offsets"),
])
def test_cross_occurrences_refusals_name_the_limit(what, kw, names):
    h, err = _create(**kw)
    assert not h
    assert names in err, err
    assert "device" not in err                       # refused before a device was looked for
    if what == "long":
        assert "query 1" in err and "257" in err
    if what == "symbols":
        assert "target 1" in err and "17" in err


def test_sixteen_symbols_per_target_pass_the_checks():
    """The limit is per target: two targets of 16 symbols each with a union of 32 get as far as the device."""
    import edlib_amd
    h, err = _create(targets=(bytes(range(65, 81)), bytes(range(97, 113))), queries=(b"A" * 256,))
    if edlib_amd.device_count() == 0:
        assert not h and "no usable HIP device" in err
    else:
        assert h, err
        edlib_amd.lib().edlibAmdBatchDestroy(h)


def test_cross_occurrences_python_checks_come_first(monkeypatch):
    import edlib_amd

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(edlib_amd, "lib", no_library)
    with pytest.raises(ValueError, match="hits=True"):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], mode="HW", k=1, hits=True, occurrences=True)
    with pytest.raises(ValueError, match="both-strand"):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], mode="HW", k=1, strands="both", occurrences=True)
    for mode in ("NW", "SHW"):
        with pytest.raises(ValueError, match="mode='HW'"):
            edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], mode=mode, k=1, occurrences=True)
    plain = edlib_amd.CrossBatch.__new__(edlib_amd.CrossBatch)
    plain._h, plain.n, plain.is_occurrences = None, 1, False
    with pytest.raises(RuntimeError, match="occurrences=True"):
        plain.occurrences()


def test_cross_occurrences_python_refusals():
    import edlib_amd
    with pytest.raises(RuntimeError, match="k must be >= 0"):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], k=-1, occurrences=True)
    with pytest.raises(RuntimeError, match="k must be >= 0"):
        edlib_amd.find_all_cross([b"ACGT"], [b"ACGT"], -1)
    with pytest.raises(RuntimeError, match="the limit is 256"):
        edlib_amd.find_all_cross([b"A" * 300], [b"ACGT"], 1)


def test_cross_occurrences_without_device_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], k=1, device=999, occurrences=True)
        return
    h, err = _create()
    assert not h
    assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], k=1, occurrences=True)
