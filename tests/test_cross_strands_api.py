"""CPU: the both-strand cross surface (edlibAmdBatchCreateCrossBothStrands / ...CrossHitsBothStrands /
edlibAmdBatchCrossStrands) and the stranded window units (edlibAmdBatchCreateWindowsStranded) are declared, exported and
laid out as documented; what they do not take is refused before any device is looked for, with the reason; the Python
guards raise; without a device Create fails loudly.  cross_strands_model() is the host statement of the strand rule the
GPU tests fold the checker's cells with; it is checked here against the oracle and a cell-by-cell restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("edlibAmdBatchCreateCrossBothStrands", "edlibAmdBatchCreateCrossHitsBothStrands", "edlibAmdBatchCrossStrands",
       "edlibAmdBatchCreateWindowsStranded")


def test_header_declares_the_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    for n in NEW:
        assert re.search(r"EDLIB_API\s+[^;(]*?\b%s\s*\(" % n, src), n
    assert "EdlibAmdCrossStrands;" in src
    body = src[src.index("typedef struct {", src.index("edlibAmdBatchCreateCrossHitsBothStrands")):src.index("EdlibAmdCrossStrands;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*[;,]", body)
    assert fields == ["numQueries", "numTargets", "numHits", "cellStrand", "hitStrand", "bestQueryStrand", "bestTargetStrand"]


def test_symbols_exported():
    import edlib_amd
    L = edlib_amd.lib()
    for n in NEW:
        assert hasattr(L, n), n


def test_cross_strands_layout():
    import edlib_amd
    V = edlib_amd.CrossStrands
    assert C.sizeof(V) == 8 + 8 + 4 * 8
    assert V.numQueries.offset == 0 and V.numTargets.offset == 4 and V.numHits.offset == 8 and V.numHits.size == 8
    for i, n in enumerate(["cellStrand", "hitStrand", "bestQueryStrand", "bestTargetStrand"]):
        assert getattr(V, n).offset == 16 + 8 * i, n


def _create_cross(name, mode="HW", task="distance", k=2):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    q = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    o = np.array([0, 4, 8], dtype=np.int64)
    h = getattr(L, name)(q.ctypes.data, o.ctypes.data, 2, q.ctypes.data, o.ctypes.data, 2, cfg, 0)
    err = edlib_amd.last_error()
    if h:
        L.edlibAmdBatchDestroy(h)
    return h, err


@pytest.mark.parametrize("name", NEW[:2])
@pytest.mark.parametrize("what,kw,words", [
    ("loc", dict(task="locations"), "DISTANCE"),
    ("path", dict(task="path"), "DISTANCE"),
    ("mode", dict(mode=7), "unknown mode"),
])
def test_cross_refusals_before_the_device(name, what, kw, words):
    h, err = _create_cross(name, **kw)
    assert not h
    assert words in err and "no usable HIP device" not in err, err


def test_hits_form_refuses_negative_k():
    h, err = _create_cross(NEW[1], k=-1)
    assert not h
    assert "k >= 0" in err and "no usable HIP device" not in err, err


def _create_windows(strand, task="distance", mode="HW", nu=None):
    import edlib_amd
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, -1, None)
    q = np.frombuffer(b"ACGTGGCA", dtype=np.uint8)
    o = np.array([0, 4, 8], dtype=np.int64)
    t = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    n = len(strand) if strand is not None else 3
    uq = np.array([0, 1, 0, 1][:n] + [0], dtype=np.int32)
    us = np.zeros(n + 1, dtype=np.int32)
    ul = np.full(n + 1, 4, dtype=np.int32)
    st = np.array(list(strand) + [0], dtype=np.uint8) if strand is not None else None
    h = L.edlibAmdBatchCreateWindowsStranded(q.ctypes.data, o.ctypes.data, 2, t.ctypes.data, 10, uq.ctypes.data,
                                             us.ctypes.data, ul.ctypes.data, st.ctypes.data if st is not None else None,
                                             n if nu is None else nu, cfg, 0)
    err = edlib_amd.last_error()
    if h:
        L.edlibAmdBatchDestroy(h)
    return h, err


def test_unit_strand_other_than_0_or_1_names_its_unit():
    h, err = _create_windows((0, 1, 2, 3))
    assert not h
    assert "unit 2 " in err and "unitStrand 2" in err and "unit 3 " not in err, err
    assert "no usable HIP device" not in err
    h, err = _create_windows((1, 0), task="path")
    assert not h and "DISTANCE" in err


def test_python_guards():
    import edlib_amd
    with pytest.raises(ValueError, match="strands"):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], strands="reverse")
    with pytest.raises(ValueError, match="strands"):
        edlib_amd.align_cross([b"ACGT"], [b"ACGT"], strands=True)
    plain = edlib_amd.CrossBatch.__new__(edlib_amd.CrossBatch)
    plain._h, plain.n, plain.is_hits = None, 1, False           # the guard answers before the handle is looked at
    with pytest.raises(RuntimeError, match="strands='both'"):
        plain.strands()
    with pytest.raises(ValueError, match="unit_strand"):
        edlib_amd.WindowBatch([b"ACGT"], b"ACGTACGTAC", [0, 0], [0, 0], [4, 4], unit_strand=[1])
    with pytest.raises(RuntimeError, match="unitStrand 2"):
        edlib_amd.WindowBatch([b"ACGT"], b"ACGTACGTAC", [0, 0], [0, 0], [4, 4], unit_strand=[1, 2])


def test_without_device_create_fails_loudly():
    """No CPU fallback: without a device (or on a device that does not exist) Create returns NULL with the reason."""
    import edlib_amd
    if edlib_amd.device_count() > 0:
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], device=999, strands="both")
        with pytest.raises(RuntimeError, match="out of range"):
            edlib_amd.WindowBatch([b"ACGT"], b"ACGTACGTAC", [0], [0], [4], device=999, unit_strand=[1])
        return
    for name in NEW[:2]:
        h, err = _create_cross(name)
        assert not h and "no usable HIP device" in err
    for strand in ((0, 1, 1), None, ()):
        h, err = _create_windows(strand)
        assert not h and "no usable HIP device" in err
    with pytest.raises(RuntimeError):
        edlib_amd.CrossBatch([b"ACGT"], [b"ACGT"], strands="both")
    with pytest.raises(RuntimeError):
        edlib_amd.align_windows([b"ACGT"], b"ACGTACGTAC", [0], [0], [4], unit_strand=[1])


# ---- the strand rule

IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]


def _cell_by_cell(fwd, rev):
    """resolve_strands() of the library's header table, one cell at a time."""
    out = {f: [] for f in fwd}
    strand = []
    for i in range(len(fwd["editDistance"])):
        df, dr = fwd["editDistance"][i], rev["editDistance"][i]
        if df >= 0 and (dr < 0 or df <= dr):
            src, s = fwd, (2 if dr == df else 0)
        elif dr >= 0:
            src, s = rev, 1
        else:
            src, s = fwd, 0
        for f in fwd:
            out[f].append(src[f][i])
        strand.append(s)
    return out, strand


@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
@pytest.mark.parametrize("k", [-1, 2])
def test_cross_strands_model_against_the_oracle(oracle, mode, k):
    from edlib_amd import cross_strands_model, reverse_complement
    rng = np.random.default_rng(["NW", "SHW", "HW"].index(mode) * 10 + k + 1)

    def rand(n, alpha=b"ACGT"):
        return bytes(rng.choice(np.frombuffer(alpha, dtype=np.uint8), size=n).astype(np.uint8))
    targets = [rand(int(n)) for n in rng.integers(4, 40, size=12)] + [b"", b"ACGT", b"TTGAATTCAA", b"ACNRTTGA"]
    queries = [b"ACGT", b"GAATTC", b"ACNRT", b"RYN", b"", b"A"]
    for i in range(7):
        t = targets[i]
        cut = t[1:1 + int(rng.integers(3, 9))]
        queries += [cut, reverse_complement(cut)]
    cells = [(q, t) for q in queries for t in targets]
    assert 190 <= len(cells) <= 400
    sides = []
    for flip in (False, True):
        r = [oracle.align(reverse_complement(q) if flip else q, t, mode, "distance", k, eq_pairs=IUPAC) for q, t in cells]
        sides.append({"editDistance": np.array([x["editDistance"] for x in r]),
                      "numLocations": np.array([x["numLocations"] for x in r]),
                      "endLocation": np.array([x["endLocations"][0] if x["numLocations"] > 0 else -1 for x in r])})
    fwd, rev = sides
    got, strand = cross_strands_model(fwd, rev)
    want, wstrand = _cell_by_cell(fwd, rev)
    for f in want:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), f
    assert strand.dtype == np.uint8 and np.array_equal(strand, wstrand)
    # the combined distance is the smaller of those within k; a palindrome ties on every target
    both = np.stack([np.where(s["editDistance"] < 0, 1 << 30, s["editDistance"]) for s in sides]).min(axis=0)
    assert np.array_equal(got["editDistance"], np.where(both == 1 << 30, -1, both))
    for i, (q, t) in enumerate(cells):
        if q in (b"ACGT", b"GAATTC"):
            assert strand[i] == (2 if fwd["editDistance"][i] >= 0 else 0)
    assert set(strand.tolist()) >= ({0, 1, 2} if k >= 0 else {1, 2})
