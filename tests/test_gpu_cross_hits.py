"""GPU: hit-list cross batches (edlibAmdBatchCreateCrossHits): the cells within k as a CSR list, with no matrix.  The list
must be exactly the cells of a dense cross batch's matrix that are not -1 (in CSR order, ascending queries), best() must
equal the dense best(), and sampled hits must equal the checker (the compiled reference where it travelled)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_cross_hits_api import best_from_hits, hits_model
from test_gpu_cross import ALPHABETS, _mixed, _pack, _rand, check_cells, ref_cells

pytestmark = pytest.mark.gpu

BEST = ("bestQuery", "bestQueryDistance", "secondQueryDistance", "bestTarget", "bestTargetDistance", "secondTargetDistance")
LIST = ("query", "editDistance", "numLocations", "endLocation")


def _hits_of(engine, queries, targets, mode, k, eqs=None):
    b = engine.CrossBatch(queries, targets, mode=mode, k=k, additionalEqualities=eqs, hits=True)
    try:
        st = b.run()
        return b.hits(), b.best(), st
    finally:
        b.close()


def _assert_same_as_dense(h, hb, m, db):
    want = hits_model(m["editDistance"], m["numLocations"], m["endLocation"])
    assert np.array_equal(h["targetOffsets"], want["targetOffsets"])
    for f in LIST:
        bad = np.nonzero(h[f] != want[f])[0]
        assert len(bad) == 0, (f, bad[:5], h[f][bad[:5]], want[f][bad[:5]])
    for f in BEST:
        assert np.array_equal(hb[f], db[f]), (f, np.nonzero(hb[f] != db[f])[0][:5])


def _check_sampled_hits(h, queries, targets, mode, k, eqs=None, n=500, seed=0):
    nh = len(h["query"])
    if nh == 0:
        return
    idx = np.random.default_rng(seed).choice(nh, size=min(n, nh), replace=False)
    t_ = np.searchsorted(h["targetOffsets"], idx, side="right") - 1
    tq = [(int(t), int(h["query"][i])) for t, i in zip(t_, idx)]
    ed, nloc, first = ref_cells(queries, targets, mode, k, eqs, tq)
    assert np.array_equal(h["editDistance"][idx], ed)
    assert np.array_equal(h["numLocations"][idx], nloc)
    assert np.array_equal(h["endLocation"][idx], first)


@pytest.mark.parametrize("alpha", sorted(ALPHABETS))
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_cross_hits_equal_dense(engine, checker, mode, alpha):
    chars, eqs = ALPHABETS[alpha]
    rng = np.random.default_rng(100 + 10 * ["NW", "SHW", "HW"].index(mode) + sorted(ALPHABETS).index(alpha))
    queries, targets = _mixed(rng, chars)
    for k in (0, 3, 20):
        d = engine.CrossBatch(queries, targets, mode=mode, k=k, additionalEqualities=eqs)
        try:
            d.run()
            m, db = d.matrix(), d.best()
        finally:
            d.close()
        h, hb, st = _hits_of(engine, queries, targets, mode, k, eqs)
        assert st["path"] & 8, st
        assert len(h["query"]) == np.count_nonzero(m["editDistance"] != -1)
        _assert_same_as_dense(h, hb, m, db)
        _check_sampled_hits(h, queries, targets, mode, k, eqs, seed=k)


def test_cross_nw_length_window(engine, checker):
    rng = np.random.default_rng(21)
    for k in (0, 1, 3, 8):
        base = [_rand(rng, int(n), b"ACGT") for n in rng.integers(20, 200, size=12)]
        queries, targets = [b""], [b""]
        for s in base:
            queries.append(s)
            for dl in (k - 1, k, k + 1):                 # |m - n| in {k - 1, k, k + 1}, longer and shorter
                if dl < 0:
                    continue
                targets.append(s + _rand(rng, dl, b"ACGT"))
                if len(s) > dl:
                    targets.append(s[:len(s) - dl])
        queries.append(_rand(rng, k + 1, b"ACGT"))      # against the empty target: |m - n| = k + 1, ed = m
        d = engine.CrossBatch(queries, targets, mode="NW", k=k)
        d.run()
        m = check_cells(d, queries, targets, "NW", k)
        db = d.best()
        d.close()
        ed = m["editDistance"]
        mlen = np.array([len(q) for q in queries]); nlen = np.array([len(t) for t in targets])
        gap = np.abs(nlen[:, None] - mlen[None, :])
        empty = (nlen[:, None] == 0) | (mlen[None, :] == 0)
        assert np.all(ed[(gap > k) & ~empty] == -1)
        assert np.all(ed[empty] == np.maximum(nlen[:, None], mlen[None, :])[empty])   # k does not apply to them
        assert np.any(ed[(gap == k) & ~empty] == k)
        h, hb, _ = _hits_of(engine, queries, targets, "NW", k)
        _assert_same_as_dense(h, hb, m, db)


def test_cross_hits_other_routes(engine, checker):
    rng = np.random.default_rng(5)
    from edlib_amd import synth
    targets = [_rand(rng, int(n), b"ACGT") for n in rng.integers(50, 500, size=30)]
    longest = max(range(30), key=lambda i: len(targets[i]))
    # a 300-base query (pair route) taken from a target, a 1 Mb target (shared-target route) among short ones
    queries = [targets[longest][:300] if len(targets[longest]) >= 300 else _rand(rng, 300, b"ACGT")]
    queries += [_rand(rng, int(n), b"ACGT") for n in rng.integers(20, 200, size=20)]
    big = synth.random_dna(11, 1_000_000)
    big = big.tobytes() if hasattr(big, "tobytes") else bytes(big)
    targets.insert(7, big)
    queries.append(big[500_000:500_120])
    queries.append(targets[3][10:60])
    for mode, k in (("HW", 8), ("NW", 200), ("SHW", 40)):
        d = engine.CrossBatch(queries, targets, mode=mode, k=k)
        d.run()
        m, db = d.matrix(), d.best()
        d.close()
        h, hb, st = _hits_of(engine, queries, targets, mode, k)
        assert st["path"] & 8
        _assert_same_as_dense(h, hb, m, db)
        _check_sampled_hits(h, queries, targets, mode, k, seed=1)
        if mode == "HW":
            s, e = h["targetOffsets"][7], h["targetOffsets"][8]
            assert len(queries) - 2 in h["query"][s:e]                  # the shared-target session's hit
            assert 0 in h["query"][h["targetOffsets"][longest + (longest >= 7)]:h["targetOffsets"][longest + (longest >= 7) + 1]]
    prot = b"ACDEFGHIKLMNPQRSTVWY"
    queries = [_rand(rng, int(n), prot) for n in rng.integers(0, 120, size=12)]
    targets = [_rand(rng, int(n), prot) for n in rng.integers(0, 400, size=9)]
    queries.append(targets[2][5:70])
    for mode, k in (("NW", 100), ("SHW", 60), ("HW", 30)):
        d = engine.CrossBatch(queries, targets, mode=mode, k=k)
        d.run()
        m = check_cells(d, queries, targets, mode, k)
        db = d.best()
        d.close()
        h, hb, st = _hits_of(engine, queries, targets, mode, k)
        assert not (st["path"] & 8)                                       # every target through the shared-target engine
        assert len(h["query"]) > 0
        _assert_same_as_dense(h, hb, m, db)


def test_cross_hits_capacity_growth(engine):
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qs = rng.choice(acgt, size=(1200, 32)).astype(np.uint8)
    ts = rng.choice(acgt, size=(1000, 32)).astype(np.uint8)
    b = engine.CrossBatch(qs, ts, mode="HW", k=32, hits=True)      # every cell within k: 1.2M hits > 2^20
    d = engine.CrossBatch(qs, ts, mode="HW", k=32)
    try:
        d.run()
        m, db = d.matrix(), d.best()
        runs = []
        for _ in range(2):
            b.run()
            runs.append((b.hits(), b.best()))
        for h, hb in runs:
            assert len(h["query"]) == 1200 * 1000
            assert np.array_equal(h["targetOffsets"], np.arange(1001, dtype=np.int64) * 1200)
            assert np.array_equal(h["query"], np.tile(np.arange(1200, dtype=np.int32), 1000))
            _assert_same_as_dense(h, hb, m, db)
    finally:
        b.close()
        d.close()


def test_cross_hits_growth_with_session_cells(engine):
    """the shape above and one target outside the kernel's envelope (65,537 bases): its 1,200 cells come from the internal
    session and go in behind the kernel's hits, here into a list that has just grown to hold both"""
    rng = np.random.default_rng(32)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qs = list(rng.choice(acgt, size=(1200, 32)).astype(np.uint8))
    ts = list(rng.choice(acgt, size=(1000, 32)).astype(np.uint8)) + [rng.choice(acgt, size=65_537).astype(np.uint8)]
    b = engine.CrossBatch(qs, ts, mode="HW", k=32, hits=True)      # every cell within k: 1,201,200 hits > 2^20
    d = engine.CrossBatch(qs, ts, mode="HW", k=32)
    try:
        d.run()
        m, db = d.matrix(), d.best()
        runs = []
        for _ in range(2):
            st = b.run()
            assert st["path"] & 1 and st["path"] & 8, st
            runs.append((b.hits(), b.best()))
        for h, hb in runs:
            assert np.array_equal(h["targetOffsets"], np.arange(1002, dtype=np.int64) * 1200)
            _assert_same_as_dense(h, hb, m, db)
    finally:
        b.close()
        d.close()


def test_cross_hits_none_and_empty(engine):
    rng = np.random.default_rng(41)
    qs = [_rand(rng, 32, b"ACGT") for _ in range(50)]
    ts = [_rand(rng, 32, b"ACGT") for _ in range(70)]
    r = engine.align_cross(qs, ts, mode="NW", k=0, hits=True)
    assert len(r["query"]) == 0 and len(r["editDistance"]) == 0
    assert np.array_equal(r["targetOffsets"], np.zeros(71, dtype=np.int64))
    for f in BEST:
        assert np.all(r[f] == -1), f
    for q, t in (([], ts), (qs, []), ([], [])):
        b = engine.CrossBatch(q, t, mode="HW", k=2, hits=True)
        b.run()
        h, hb = b.hits(), b.best()
        assert len(h["query"]) == 0 and np.array_equal(h["targetOffsets"], np.zeros(len(t) + 1, dtype=np.int64))
        assert len(hb["bestQuery"]) == len(t) and len(hb["bestTarget"]) == len(q)
        b.close()


def test_cross_hits_views_and_refusals(engine):
    import ctypes as C
    L = engine.lib()
    h = engine.CrossBatch([b"ACGT", b"GGA"], [b"ACGTACGT", b"TTT", b""], mode="HW", k=1, hits=True)
    v = engine.CrossHits()
    assert L.edlibAmdBatchCrossHits(h._h, C.byref(v)) != 0                 # before the first Run
    assert "Run" in engine.last_error()
    h.run()
    with pytest.raises(RuntimeError, match="without hits"):
        h.matrix()
    cv = engine.CrossView()
    assert L.edlibAmdBatchCrossView(h._h, engine.CROSS_MATRIX, C.byref(cv)) != 0
    assert "hit-list" in engine.last_error()
    assert L.edlibAmdBatchCrossView(h._h, engine.CROSS_BEST, C.byref(cv)) == 0
    assert L.edlibAmdBatchResultsView(h._h, C.byref(engine.ResultsView())) != 0
    assert "cross" in engine.last_error()
    assert L.edlibAmdBatchResultsFlat(h._h, *([None] * 9)) != 0
    got = h.hits()
    s, e = got["targetOffsets"][2], got["targetOffsets"][3]                # empty target: every query a hit, ed = m > k
    assert e == len(got["query"]) and got["query"][s:e].tolist() == [0, 1] and got["editDistance"][s:e].tolist() == [4, 3]
    d = engine.CrossBatch([b"ACGT", b"GGA"], [b"ACGTACGT", b"TTT", b""], mode="HW", k=1)
    d.run()
    _assert_same_as_dense(got, h.best(), d.matrix(), d.best())
    h.close()
    assert L.edlibAmdBatchCrossHits(d._h, C.byref(v)) != 0                 # a dense batch has no hit list
    assert "not a hit-list" in engine.last_error()
    d.close()


def test_cross_hits_at_size(engine, checker):
    """200,000 x 200,000 32-base sequences, NW, k = 2: the dense matrix would need 480 GB."""
    rng = np.random.default_rng(51)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    nfam, kids, L = 2000, 100, 32
    parents = rng.choice(acgt, size=(nfam, L)).astype(np.uint8)
    seqs = np.repeat(parents, kids, axis=0)
    for j in range(1, 3):                                  # 0-2 substitutions per child
        hit = rng.random(len(seqs)) < (0.8 if j == 1 else 0.5)
        pos = rng.integers(0, L, size=len(seqs))
        seqs[hit, pos[hit]] = rng.choice(acgt, size=int(hit.sum()))
    b = engine.CrossBatch(seqs, seqs, mode="NW", k=2, hits=True)
    try:
        st = b.run()
        h, hb = b.hits(), b.best()
    finally:
        b.close()
    n = len(seqs)
    nh = len(h["query"])
    assert st["path"] & 8 and h["targetOffsets"][-1] == nh and nh >= n
    # 20 whole families against a dense batch over their 2,000 members
    fams = np.sort(rng.choice(nfam, size=20, replace=False))
    members = (fams[:, None] * kids + np.arange(kids)[None, :]).reshape(-1)
    d = engine.CrossBatch(seqs[members], seqs[members], mode="NW", k=2)
    d.run()
    dm = d.matrix()["editDistance"]
    d.close()
    pos = np.full(n, -1, dtype=np.int64)
    pos[members] = np.arange(len(members))
    t_all = np.repeat(np.arange(n), np.diff(h["targetOffsets"]))
    inside = (pos[t_all] >= 0) & (pos[h["query"]] >= 0)
    sub = np.full(dm.shape, -1, dtype=np.int32)
    sub[pos[t_all[inside]], pos[h["query"][inside]]] = h["editDistance"][inside]
    assert np.array_equal(sub, dm)
    # 20,000 sampled hits against the checker
    idx = rng.choice(nh, size=min(20_000, nh), replace=False)
    qs = [seqs[int(h["query"][i])].tobytes() for i in idx]
    ts = [seqs[int(t_all[i])].tobytes() for i in idx]
    qp, qo = _pack(qs)
    tp, to = _pack(ts)
    r = O.pool_align(qp, qo, tp, to, False, "NW", "distance", 2)
    assert np.array_equal(np.asarray(r["editDistance"]), h["editDistance"][idx])
    # best hits against a numpy reduction of the list
    want = best_from_hits(h, n)
    for f in BEST:
        assert np.array_equal(hb[f], want[f]), f
