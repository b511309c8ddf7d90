"""GPU: self batches (edlibAmdBatchCreateSelf / CreateSelfHits): one set against itself, every unordered pair once.  Every
distance checked is compared with the checker (the compiled reference where it travelled) over the i < j pairs; the hit
list with the dense batch's cells within k; nearest() with self_nearest_model() fed with the reference's distances; the
counters with the numpy formulas of test_self_model.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_cross import IUPAC, _pack, _rand
from test_self_model import self_cells, self_word_steps

pytestmark = pytest.mark.gpu

NEAR = ("nearest", "nearestDistance", "secondDistance")


def ref_pairs(seqs, i, j, k, eqs=None):
    """editDistance of edlibAlign(seqs[i], seqs[j], NW, k) for the listed pairs, by the checker."""
    if len(i) == 0:
        return np.zeros(0, dtype=np.int32)
    qp, qo = _pack([bytes(seqs[int(a)]) for a in i])
    tp, to = _pack([bytes(seqs[int(b)]) for b in j])
    r = O.pool_align(qp, qo, tp, to, False, "NW", "distance", k, eq_pairs=eqs)
    return np.asarray(r["editDistance"]).astype(np.int32)


def ref_condensed(seqs, k, eqs=None):
    i, j = np.triu_indices(len(seqs), 1)
    return ref_pairs(seqs, i, j, k, eqs)


def csr_of(n, cond):
    """The hit list of a condensed vector: the pairs that are not -1, by row, partners ascending."""
    i, j = np.triu_indices(n, 1)
    keep = cond != -1
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i[keep], minlength=n), out=off[1:])
    return {"rowOffsets": off, "partner": j[keep].astype(np.int32), "editDistance": cond[keep].astype(np.int32)}


def run_dense(engine, seqs, k, eqs=None):
    b = engine.SelfBatch(seqs, k=k, additionalEqualities=eqs)
    try:
        st = b.run()
        return b.condensed(), b.nearest(), st
    finally:
        b.close()


def run_hits(engine, seqs, k, eqs=None):
    b = engine.SelfBatch(seqs, k=k, additionalEqualities=eqs, hits=True)
    try:
        st = b.run()
        return b.hits(), b.nearest(), st
    finally:
        b.close()


def assert_csr(h, n, want):
    """rows ascending, every pair once, no self pair, equal to the wanted list"""
    off, p = h["rowOffsets"], h["partner"]
    assert off[0] == 0 and off[-1] == len(p) == len(h["editDistance"]) and np.all(np.diff(off) >= 0)
    row = np.repeat(np.arange(n), np.diff(off))
    assert np.all(p > row) and np.all(p < n)                       # j > i: no self pair, no pair twice across rows
    same = row[1:] == row[:-1]
    assert np.all(p[1:][same] > p[:-1][same])                      # ascending, so none twice inside a row
    assert np.array_equal(off, want["rowOffsets"])
    for f in ("partner", "editDistance"):
        bad = np.nonzero(h[f] != want[f])[0]
        assert len(bad) == 0, (f, bad[:5], h[f][bad[:5]], want[f][bad[:5]])


def assert_nearest(engine, got, n, cond):
    i, j = np.triu_indices(n, 1)
    want = engine.self_nearest_model(n, i, j, cond)
    for f in NEAR:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def assert_dense(engine, seqs, k, want, eqs=None, word_steps=True):
    cond, near, st = run_dense(engine, seqs, k, eqs)
    n = len(seqs)
    assert cond.dtype == np.int32 and cond.shape == (n * (n - 1) // 2,)
    bad = np.nonzero(cond != want)[0]
    i, j = np.triu_indices(n, 1)
    assert len(bad) == 0, (k, [(int(i[b]), int(j[b]), int(cond[b]), int(want[b]), len(seqs[i[b]]), len(seqs[j[b]])) for b in bad[:5]])
    assert_nearest(engine, near, n, want)
    lens = [len(s) for s in seqs]
    assert st["cells"] == self_cells(lens)
    if word_steps:
        assert st["word_steps"] == self_word_steps(lens, k)
    return cond, st


def assert_hits(engine, seqs, k, want, eqs=None):
    h, near, st = run_hits(engine, seqs, k, eqs)
    assert_csr(h, len(seqs), csr_of(len(seqs), want))
    assert_nearest(engine, near, len(seqs), want)
    lens = [len(s) for s in seqs]
    assert st["cells"] == self_cells(lens) and st["word_steps"] == self_word_steps(lens, k)
    return h, st


_MIXED = {}


def mixed():
    """200 sequences of 1..90 bases (one, two and three words): 20 exact duplicates, 10 of one length, two empty; and the
    reference's condensed distances at the k the tests use, computed once."""
    if not _MIXED:
        rng = np.random.default_rng(7)
        seqs = [_rand(rng, int(m), b"ACGT") for m in rng.integers(1, 91, size=168)]
        seqs[0], seqs[1], seqs[2] = _rand(rng, 1, b"ACGT"), _rand(rng, 90, b"ACGT"), _rand(rng, 33, b"ACGT")
        seqs[3] = _rand(rng, 60, b"ACGT")                                   # with two close relatives
        seqs[4], seqs[5] = seqs[3][:-1], seqs[3][:30] + b"A" + seqs[3][30:]
        seqs += [_rand(rng, 47, b"ACGT") for _ in range(10)]              # rank ties
        seqs += [seqs[int(s)] for s in rng.integers(0, len(seqs), size=20)]   # exact duplicates
        seqs += [b"", b""]
        order = rng.permutation(len(seqs))
        seqs = [seqs[int(o)] for o in order]
        _MIXED["seqs"] = seqs
        _MIXED["ref"] = {k: ref_condensed(seqs, k) for k in (-1, 0, 3)}
    return _MIXED["seqs"], _MIXED["ref"]


@pytest.mark.parametrize("k", [-1, 3])
def test_self_mixed_dense(engine, checker, k):
    seqs, ref = mixed()
    assert len(seqs) == 200 and max(map(len, seqs)) == 90 and sum(1 for s in seqs if not s) == 2
    _, st = assert_dense(engine, seqs, k, ref[k])
    assert st["path"] & 8 and st["scan_launches"] == 3


@pytest.mark.parametrize("k", [0, 3])
def test_self_mixed_hits(engine, checker, k):
    seqs, ref = mixed()
    h, st = assert_hits(engine, seqs, k, ref[k])
    assert st["path"] & 8
    assert len(h["partner"]) >= 20 + 2 * 198 - 1                  # the duplicates, and every pair with an empty sequence
    if k == 3:                                                      # equal to the dense batch's cells that are not -1
        cond, _, _ = run_dense(engine, seqs, 3)
        assert_csr(h, len(seqs), csr_of(len(seqs), cond))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 96, 129])
def test_self_tile_edges(engine, checker, n):
    rng = np.random.default_rng(n)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    arr = rng.choice(acgt, size=(n, 24)).astype(np.uint8)
    arr[n // 2] = arr[0]
    seqs = [bytes(r) for r in arr]
    want = ref_condensed(seqs, -1)
    cond, st = assert_dense(engine, seqs, -1, want)
    assert st["word_steps"] == n * (n - 1) // 2 * 24
    assert_hits(engine, seqs, 8, ref_condensed(seqs, 8))
    if n == 96:
        c = engine.CrossBatch(seqs, seqs, "NW")
        try:
            cst = c.run()
            m = c.matrix()["editDistance"]
        finally:
            c.close()
        i, j = np.triu_indices(n, 1)
        assert np.array_equal(m[j, i], cond)                       # cell (query i, target j)
        assert 2 * st["word_steps"] + 96 * 24 == cst["word_steps"]


def test_self_work_items(engine, checker):
    """4,096 sequences: 64 query tiles whose ranges are cut into several work items each, most starting mid-range."""
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = np.repeat(rng.choice(acgt, size=(64, 32)).astype(np.uint8), 64, axis=0)
    for _ in range(2):
        pos = rng.integers(0, 32, size=len(seqs))
        seqs[np.arange(len(seqs)), pos] = rng.choice(acgt, size=len(seqs))
    seqs = seqs[rng.permutation(len(seqs))]
    n = len(seqs)
    h, near, st = run_hits(engine, seqs, 2)
    c = engine.CrossBatch(seqs, seqs, "NW", k=2, hits=True)
    try:
        cst = c.run()
        ch = c.hits()
    finally:
        c.close()
    t = np.repeat(np.arange(n), np.diff(ch["targetOffsets"]))
    q = ch["query"].astype(np.int64)
    up = q < t                                                      # query i against target j, i < j
    order = np.lexsort((t[up], q[up]))
    want = {"rowOffsets": np.concatenate([[0], np.cumsum(np.bincount(q[up], minlength=n))]).astype(np.int64),
            "partner": t[up][order].astype(np.int32), "editDistance": ch["editDistance"][up][order]}
    assert_csr(h, n, want)
    assert st["word_steps"] == n * (n - 1) // 2 * 32 and 2 * st["word_steps"] + n * 32 == cst["word_steps"]
    # 2,000 sampled pairs against the reference: half of them hits, half anywhere in the triangle
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    pick = rng.choice(len(row), size=1000, replace=False)
    assert np.array_equal(ref_pairs(seqs, row[pick], h["partner"][pick], 2), h["editDistance"][pick])
    i = rng.integers(0, n - 1, size=1000)
    j = np.minimum(i + 1 + rng.integers(0, n, size=1000) % (n - 1 - i), n - 1)
    got = np.full(1000, -1, dtype=np.int32)
    keys = row.astype(np.int64) * n + h["partner"]
    at = np.searchsorted(keys, i * n + j)
    found = (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == i * n + j)
    got[found] = h["editDistance"][at[found]]
    assert np.array_equal(ref_pairs(seqs, i, j, 2), got)
    i, j = row, h["partner"]
    want_near = engine.self_nearest_model(n, i, j, h["editDistance"])
    for f in NEAR:
        assert np.array_equal(near[f], want_near[f]), f


def test_self_length_window(engine, checker):
    rng = np.random.default_rng(13)
    base = _rand(rng, 60, b"ACGT")
    seqs = []
    for m in rng.integers(20, 61, size=300):
        s = bytearray(base[:int(m)])
        for p in rng.integers(0, int(m), size=int(rng.integers(0, 3))):
            s[int(p)] = b"ACGT"[int(rng.integers(0, 4))]
        seqs.append(bytes(s))
    want = ref_condensed(seqs, 2)
    lens = np.array([len(s) for s in seqs])
    i, j = np.triu_indices(len(seqs), 1)
    assert np.all(want[np.abs(lens[i] - lens[j]) > 2] == -1) and np.count_nonzero(want != -1) > 300
    _, st = assert_dense(engine, seqs, 2, want)
    inside = np.abs(lens[i] - lens[j]) <= 2
    assert st["word_steps"] == int((((np.minimum(lens[i], lens[j]) + 31) // 32) * np.maximum(lens[i], lens[j]))[inside].sum())
    assert_hits(engine, seqs, 2, want)


@pytest.mark.parametrize("alpha", ["ACGTN", "ACGTRYKMN", "IUPAC"])
def test_self_alphabets_and_equalities(engine, checker, alpha):
    chars, eqs = (b"ACGTN", IUPAC) if alpha == "IUPAC" else (alpha.encode(), None)
    rng = np.random.default_rng(len(alpha) + (eqs is not None))
    base = _rand(rng, 70, chars)
    seqs = []
    for m in rng.integers(5, 71, size=80):
        s = bytearray(base[:int(m)])
        for p in rng.integers(0, int(m), size=2):
            s[int(p)] = chars[int(rng.integers(0, len(chars)))]
        seqs.append(bytes(s))
    for k in (-1, 4):
        want = ref_condensed(seqs, k, eqs)
        _, st = assert_dense(engine, seqs, k, want, eqs)
        assert st["path"] & 8
    assert_hits(engine, seqs, 4, want, eqs)


def test_self_other_routes(engine, checker):
    rng = np.random.default_rng(17)
    seqs = [_rand(rng, int(m), b"ACGT") for m in rng.integers(1, 200, size=37)]
    long_ = _rand(rng, 300, b"ACGT")
    seqs[5], seqs[20] = long_, long_[:150] + b"T" + long_[150:299]
    seqs += [_rand(rng, 300, b"ACGT"), b"", seqs[7]]
    assert len(seqs) == 40 and sum(1 for s in seqs if len(s) == 300) == 3
    for k in (-1, 5):
        want = ref_condensed(seqs, k)
        _, st = assert_dense(engine, seqs, k, want)
        assert st["path"] & 8 and st["path"] & 2                    # the kernel and the internal pair batch
    h, st = assert_hits(engine, seqs, 5, want)
    assert st["path"] & 2
    assert 20 in h["partner"][h["rowOffsets"][5]:h["rowOffsets"][6]]   # the pair batch's hit
    prot = b"ACDEFGHIKLMNPQRST"                                       # 17 symbols: every pair through the pair batch
    seqs = [_rand(rng, int(m), prot) for m in rng.integers(0, 80, size=10)] + [prot, prot[:-1]]
    for k in (-1, 3):
        want = ref_condensed(seqs, k)
        _, st = assert_dense(engine, seqs, k, want, word_steps=False)
        assert not (st["path"] & 8) and st["path"] & 2
    assert_csr(run_hits(engine, seqs, 3)[0], len(seqs), csr_of(len(seqs), want))


@pytest.mark.parametrize("seqs", [[], [b"ACGT"], [b""], [b"", b""]])
def test_self_without_a_pair(engine, seqs):
    n = len(seqs)
    cond, near, st = run_dense(engine, seqs, -1)
    assert cond.shape == (n * (n - 1) // 2,) and st["word_steps"] == 0 and st["cells"] == 0
    assert cond.tolist() == ([0] if n == 2 else [])
    h, hnear, _ = run_hits(engine, seqs, 1)
    assert np.array_equal(h["rowOffsets"], np.array([0] + ([1, 1] if n == 2 else [0] * n), dtype=np.int64))
    want = {"nearest": [1, 0], "nearestDistance": [0, 0], "secondDistance": [-1, -1]} if n == 2 else {f: [-1] * n for f in NEAR}
    for got in (near, hnear):
        for f in NEAR:
            assert got[f].tolist() == want[f], f


def test_self_hits_capacity_growth(engine):
    seq = b"ACGTTGCAACGTACGTTGCA"
    n = 2048
    b = engine.SelfBatch([seq] * n, k=0, hits=True)                    # 2,096,128 hits, past the 2^20 the list starts at
    try:
        runs = []
        for _ in range(2):
            b.run()
            runs.append((b.hits(), b.nearest()))
    finally:
        b.close()
    i, j = np.triu_indices(n, 1)
    for h, near in runs:
        assert len(h["partner"]) == n * (n - 1) // 2 == 2_096_128
        assert np.array_equal(h["rowOffsets"][1:], np.cumsum(np.arange(n - 1, -1, -1)))
        assert np.array_equal(h["partner"], j) and not h["editDistance"].any()
        assert near["nearest"].tolist() == [1] + [0] * (n - 1)
        assert not near["nearestDistance"].any() and not near["secondDistance"].any()


def test_self_one_shots(engine, checker):
    seqs, ref = mixed()
    assert np.array_equal(engine.pdist(seqs), ref[-1])
    assert np.array_equal(engine.pdist(seqs, k=3), ref[3])
    r = engine.pairs_within(seqs, 3)
    h, near, _ = run_hits(engine, seqs, 3)
    for f in ("rowOffsets", "partner", "editDistance"):
        assert np.array_equal(r[f], h[f]), f
    for f in NEAR:
        assert np.array_equal(r[f], near[f]), f
    assert engine.pdist([b"AC", b"AG", b"ACGT"]).tolist() == [1, 2, 2]


def test_self_views_and_refusals(engine):
    L = engine.lib()
    d = engine.SelfBatch([b"ACGT", b"ACGA", b"TTGA"], k=2)
    h = engine.SelfBatch([b"ACGT", b"ACGA", b"TTGA"], k=2, hits=True)
    try:
        v, hv = engine.SelfView(), engine.SelfHits()
        assert L.edlibAmdBatchSelfView(d._h, engine.SELF_NEAREST, C.byref(v)) != 0      # before the first Run
        assert "Run" in engine.last_error()
        d.run()
        h.run()
        assert L.edlibAmdBatchSelfView(d._h, engine.SELF_NEAREST, C.byref(v)) == 0
        assert v.numSequences == 3 and v.numPairs == 3 and not v.editDistance and v.nearest
        assert L.edlibAmdBatchSelfView(d._h, 4, C.byref(v)) != 0
        assert L.edlibAmdBatchSelfView(h._h, engine.SELF_DISTANCES | engine.SELF_NEAREST, C.byref(v)) == 0
        assert not v.editDistance and v.nearest                      # a hit-list batch keeps no condensed vector
        with pytest.raises(RuntimeError, match="without hits"):
            h.condensed()
        assert L.edlibAmdBatchSelfHits(d._h, C.byref(hv)) != 0
        assert "not a hit-list" in engine.last_error()
        for b in (d, h):                                             # every other view names the self views
            for call in (lambda: L.edlibAmdBatchResultsView(b._h, C.byref(engine.ResultsView())),
                         lambda: L.edlibAmdBatchResultsFlat(b._h, *([None] * 9)),
                         lambda: L.edlibAmdBatchCrossView(b._h, engine.CROSS_BEST, C.byref(engine.CrossView())),
                         lambda: L.edlibAmdBatchCrossHits(b._h, C.byref(engine.CrossHits())),
                         lambda: L.edlibAmdBatchCrossStrands(b._h, engine.CROSS_BEST, C.byref(engine.CrossStrands())),
                         lambda: L.edlibAmdBatchStrandView(b._h, C.byref(engine.StrandView())),
                         lambda: L.edlibAmdBatchSharedHits(b._h, C.byref(engine.ReadHits())),
                         lambda: L.edlibAmdBatchWindowView(b._h, engine.WINDOW_BEST, C.byref(engine.WindowView()))):
                assert call() != 0
                assert "edlibAmdBatchSelfView" in engine.last_error(), engine.last_error()
        c = engine.CrossBatch([b"ACGT"], [b"ACGA"], "NW")
        c.run()
        assert L.edlibAmdBatchSelfView(c._h, engine.SELF_NEAREST, C.byref(v)) != 0
        assert "not a self batch" in engine.last_error()
        c.close()
        assert d.condensed().tolist() == [1, -1, 2] and h.hits()["partner"].tolist() == [1, 2]
    finally:
        d.close()
        h.close()
