"""CPU: the window-batch surface (edlibAmdBatchCreateWindows / edlibAmdBatchWindowView) is declared, exported and laid
out as documented; Create refuses a bad task or a bad unit list before it looks for a device, naming the first bad unit,
and without a device a valid Create fails loudly.  window_best_model() is the numpy statement of the best-unit rules
the GPU tests compare best() with; it is checked here against a brute force."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_window_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in ("edlibAmdBatchCreateWindows", "edlibAmdBatchWindowView"):
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    assert "EdlibAmdWindowView;" in src
    assert re.search(r"#define\s+EDLIB_AMD_WINDOW_UNITS\s+1\b", src)
    assert re.search(r"#define\s+EDLIB_AMD_WINDOW_BEST\s+2\b", src)
    assert re.search(r"bit 4 \(value 16\)[^\n]*window kernel", src)


def test_window_symbols_exported():
    import edlib_amd
    L = edlib_amd.lib()
    assert hasattr(L, "edlibAmdBatchCreateWindows") and hasattr(L, "edlibAmdBatchWindowView")


def test_window_view_layout():
    import edlib_amd
    V = edlib_amd.WindowView
    assert C.sizeof(V) == 8 + 6 * 8
    assert V.numUnits.offset == 0 and V.numQueries.offset == 4
    names = ["editDistance", "numLocations", "endLocation", "bestUnit", "bestDistance", "secondDistance"]
    for i, n in enumerate(names):
        assert getattr(V, n).offset == 8 + 8 * i, n
    assert edlib_amd.WINDOW_UNITS == 1 and edlib_amd.WINDOW_BEST == 2


QUERIES = b"ACGTACGT"                       # two queries of 4 bases
TARGET = b"ACGTTGCAAC"                      # 10 bases


def _create(task="distance", uq=(0, 1), us=(0, 6), ul=(4, 4), num_units=None, target_length=len(TARGET)):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config("HW", task, -1, None)
    q = np.frombuffer(QUERIES, dtype=np.uint8)
    o = np.array([0, 4, 8], dtype=np.int64)
    t = np.frombuffer(TARGET, dtype=np.uint8)
    a = [np.array(list(x) + [0], dtype=np.int32) for x in (uq, us, ul)]
    n = len(uq) if num_units is None else num_units
    h = L.edlibAmdBatchCreateWindows(q.ctypes.data, o.ctypes.data, 2, t.ctypes.data, target_length,
                                     a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, n, cfg, 0)
    err = edlib_amd.last_error()
    if h:
        L.edlibAmdBatchDestroy(h)
    return h, err


@pytest.mark.parametrize("task", ["locations", "path"])
def test_windows_refuse_other_tasks(task):
    h, err = _create(task)
    assert not h
    assert "DISTANCE" in err


def test_windows_refuse_negative_unit_count():
    h, err = _create(num_units=-1)
    assert not h
    assert "numUnits" in err


INT_MAX = 2**31 - 1
BAD_UNITS = {
    # name: (unitQuery, unitStart, unitLength), index of the first bad unit, words of the message
    "query_below": (((0, -1), (0, 0), (4, 4)), 1, ["unit 1", "query -1", "numQueries"]),
    "query_above": (((2, 0), (0, 0), (4, 4)), 0, ["unit 0", "query 2", "numQueries"]),
    "start_negative": (((0, 1, 0), (0, 0, -3), (4, 4, 2)), 2, ["unit 2", "unitStart", "-3"]),
    "length_negative": (((0, 1), (0, 0), (-1, 4)), 0, ["unit 0", "unitLength", "-1"]),
    "past_the_end": (((0, 1), (0, 7), (10, 4)), 1, ["unit 1", "targetLength", "7", "4"]),
    "past_the_end_by_one": (((0,), (1,), (10,)), 0, ["unit 0", "targetLength"]),
    "sum_overflows_32_bits": (((0, 0), (0, INT_MAX), (10, INT_MAX)), 1, ["unit 1", "targetLength"]),
    "first_of_two_bad": (((0, 5, 0, 9), (0, 0, -1, 0), (4, 4, 4, 4)), 1, ["unit 1", "query 5"]),
    "first_of_two_kinds": (((0, 0, 7), (0, 8, 0), (4, 4, 4)), 1, ["unit 1", "targetLength"]),
}


@pytest.mark.parametrize("name", sorted(BAD_UNITS))
def test_windows_refuse_bad_units(name):
    (uq, us, ul), first, words = BAD_UNITS[name]
    h, err = _create(uq=uq, us=us, ul=ul)
    assert not h
    assert "no usable HIP device" not in err, err
    for w in words:
        assert w in err, (w, err)
    others = [i for i in range(len(uq)) if i != first]
    for i in others:
        assert "unit %d " % i not in err, err


def test_unit_lists_must_agree_in_length():
    import edlib_amd
    with pytest.raises(ValueError):
        edlib_amd.WindowBatch([b"ACGT"], TARGET, [0, 0], [0], [4, 4])


def test_windows_without_device_fail_loudly():
    """No CPU fallback: a valid unit list (an empty one too) gets as far as the device check."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.WindowBatch([b"ACGT"], TARGET, [0], [0], [4], device=999)
        return
    for kw in ({}, {"uq": (), "us": (), "ul": ()}, {"uq": (0,), "us": (10,), "ul": (0,)}):
        h, err = _create(**kw)
        assert not h
        assert "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.WindowBatch([b"ACGT"], TARGET, [0], [0], [4])


def _brute(unit_query, ed, nq):
    out = {f: np.full(nq, -1, dtype=np.int32) for f in ("bestUnit", "bestDistance", "secondDistance")}
    for q in range(nq):
        live = [(int(ed[u]), u) for u in range(len(ed)) if unit_query[u] == q and ed[u] >= 0]
        if not live:
            continue
        d, u = min(live)
        others = [x for x, j in live if j != u]
        out["bestUnit"][q], out["bestDistance"][q] = u, d
        out["secondDistance"][q] = min(others) if others else -1
    return out


@pytest.mark.parametrize("nu,nq", [(0, 0), (0, 3), (1, 1), (40, 6), (300, 17), (64, 1)])
def test_window_best_model_matches_brute_force(nu, nq):
    from edlib_amd import window_best_model
    rng = np.random.default_rng(nu * 100 + nq)
    uq = rng.integers(0, max(nq, 1), size=nu).astype(np.int32)
    ed = rng.integers(-1, 4, size=nu).astype(np.int32)              # many ties and -1 units
    if nq > 3:
        uq[uq == 1] = 0                                             # query 1: no unit at all
        ed[uq == 2] = -1                                            # query 2: every unit above k
        ed[uq == 3] = 2                                             # query 3: one distance, ties all the way
    want = _brute(uq, ed, nq)
    got = window_best_model(uq, ed, nq)
    for f in want:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), f
    if nq > 3:
        assert want["bestUnit"][1] == -1 and want["bestUnit"][2] == -1
        if (uq == 3).sum() > 1:
            assert want["secondDistance"][3] == want["bestDistance"][3] == 2
