"""GPU: cross batches on both strands (edlibAmdBatchCreateCrossBothStrands / ...CrossHitsBothStrands).  The expected cells
come from the checker (the compiled reference where it travelled) over the expanded pairs of both strands -- every query
and reverse_complement(query) against every target --, folded with cross_strands_model(); the best hits from best_model()
on the folded matrix.  Every cell of every case is checked."""
import ctypes as C

import numpy as np
import pytest

import edlib_amd
from edlib_amd import cross_strands_model, reverse_complement
from test_cross_api import best_model
from test_cross_hits_api import hits_model
from test_gpu_cross import IUPAC, _rand, ref_cells

pytestmark = pytest.mark.gpu

FIELDS = ("editDistance", "numLocations", "endLocation")
BEST = ("bestQuery", "bestQueryDistance", "secondQueryDistance", "bestTarget", "bestTargetDistance", "secondTargetDistance")


def ref_both(queries, targets, mode, k, eqs=None):
    """(fwd, rev, cells, strand): the checker's matrices (numTargets, numQueries) of the queries and of their reverse
    complements, and their fold."""
    nt, nq = len(targets), len(queries)
    tq = [(t, q) for t in range(nt) for q in range(nq)]
    out = []
    for qs in (queries, [reverse_complement(q) for q in queries]):
        ed, nloc, first = ref_cells(qs, targets, mode, k, eqs, tq)
        out.append({f: np.asarray(v).reshape(nt, nq) for f, v in zip(FIELDS, (ed, nloc, first))})
    cells, strand = cross_strands_model(out[0], out[1])
    return out[0], out[1], cells, strand


def best_strands_model(ed, strand):
    b = best_model(ed)
    nt, nq = ed.shape
    bq, bt = b["bestQuery"], b["bestTarget"]
    sq = np.where(bq >= 0, strand[np.arange(nt), np.maximum(bq, 0)], 0).astype(np.uint8) if nq else np.zeros(nt, np.uint8)
    st = np.where(bt >= 0, strand[np.maximum(bt, 0), np.arange(nq)], 0).astype(np.uint8) if nt else np.zeros(nq, np.uint8)
    return b, sq, st


def check_both(engine, queries, targets, mode, k, eqs=None, runs=1):
    """A dense both-strand batch against the folded reference: every cell, the strand bytes, the best arrays.  Returns
    (matrix, strands, best, stats, fwd, rev)."""
    fwd, rev, cells, strand = ref_both(queries, targets, mode, k, eqs)
    b = engine.CrossBatch(queries, targets, mode=mode, k=k, additionalEqualities=eqs, strands="both")
    try:
        views = []
        for _ in range(runs):
            st = b.run()
            views.append((b.matrix(), b.strands(), b.best()))
    finally:
        b.close()
    m, s, best = views[0]
    for other in views[1:]:                          # every Run gives identical views
        for a, c in zip(views[0], other):
            for f in a:
                assert np.array_equal(a[f], c[f]), f
    for f in FIELDS:
        bad = np.argwhere(m[f] != cells[f])
        assert len(bad) == 0, (f, mode, k, [(tuple(i), int(m[f][tuple(i)]), int(cells[f][tuple(i)]),
                                             len(queries[i[1]]), len(targets[i[0]])) for i in bad[:5]])
    bad = np.argwhere(s["cellStrand"] != strand)
    assert s["cellStrand"].dtype == np.uint8 and len(bad) == 0, (mode, k, [(tuple(i), int(s["cellStrand"][tuple(i)]),
                                                                             int(strand[tuple(i)])) for i in bad[:5]])
    want, sq, stt = best_strands_model(cells["editDistance"], strand)
    for f in BEST:
        assert np.array_equal(best[f], want[f]), (f, np.nonzero(best[f] != want[f])[0][:5])
    assert np.array_equal(s["bestQueryStrand"], sq) and np.array_equal(s["bestTargetStrand"], stt)
    assert st["cells"] == 2 * sum(map(len, queries)) * sum(map(len, targets))
    return m, s, best, st, fwd, rev


def check_hits_equal_dense(engine, queries, targets, mode, k, m, s, best, eqs=None, runs=1):
    h = engine.CrossBatch(queries, targets, mode=mode, k=k, additionalEqualities=eqs, hits=True, strands="both")
    try:
        for _ in range(runs):
            st = h.run()
            got, hs, hb = h.hits(), h.strands(), h.best()
    finally:
        h.close()
    want = hits_model(m["editDistance"], m["numLocations"], m["endLocation"])
    assert np.array_equal(got["targetOffsets"], want["targetOffsets"])
    for f in ("query",) + FIELDS:
        assert np.array_equal(got[f], want[f]), (f, mode, k)
    t, q = np.nonzero(m["editDistance"] != -1)
    assert np.array_equal(hs["hitStrand"], s["cellStrand"][t, q])
    for f in BEST:
        assert np.array_equal(hb[f], best[f]), (f, mode, k)
    assert np.array_equal(hs["bestQueryStrand"], s["bestQueryStrand"])
    assert np.array_equal(hs["bestTargetStrand"], s["bestTargetStrand"])
    return st


def _mutate(rng, s, edits, alpha=b"ACGT"):
    s = bytearray(s)
    for _ in range(edits):
        if s:
            s[int(rng.integers(0, len(s)))] = int(rng.choice(np.frombuffer(alpha, dtype=np.uint8)))
    return bytes(s)


def _planted(rng, alpha=b"ACGT", nq=40, nt=120, tmax=600, lower=False):
    """nq queries of every word count (and an empty one) against nt targets of 0 .. tmax columns: a third of the queries
    are cut from a target, a third from a target's reverse complement; a few targets are (mutated) copies of a query or
    of its reverse complement, so that NW finds cells within a small k on either strand."""
    qlens = [1, 31, 32, 33, 64, 65, 128, 255, 256, 0] + [int(n) for n in rng.integers(1, 257, size=nq - 10)]
    tlens = [0, 1, tmax] + [int(n) for n in rng.integers(260, tmax + 1, size=nt - 3 - 16)]
    targets = [_rand(rng, n, alpha) for n in tlens]
    queries = []
    for i, n in enumerate(qlens):
        t = targets[3 + i % (len(targets) - 3)]
        s = int(rng.integers(0, len(t) - n + 1))
        if n and i % 3 == 0:
            queries.append(_mutate(rng, t[s:s + n], i % 4, alpha))
        elif n and i % 3 == 1:
            queries.append(reverse_complement(_mutate(rng, t[s:s + n], i % 4, alpha)))
        else:
            queries.append(_rand(rng, n, alpha))
    for j in range(8):                               # whole-length relatives, for NW
        q = queries[(5 * j + 2) % nq]
        targets.append(_mutate(rng, q, j % 3, alpha))
        targets.append(_mutate(rng, reverse_complement(q), j % 3, alpha))
    if lower:
        queries = [q.lower() if i % 2 else q for i, q in enumerate(queries)]
        targets = [t.lower() if i % 3 == 0 else t for i, t in enumerate(targets)]
    return queries, targets


def _kinds(fwd, rev):
    f, r = fwd["editDistance"] >= 0, rev["editDistance"] >= 0
    return {"forward": bool((f & ~r).any()), "reverse": bool((~f & r).any()), "both": bool((f & r).any()),
            "neither": bool((~f & ~r).any())}


# ---- 1. tile shapes: qt = 2 .. 64, ragged last tiles whose padding is mate pairs

@pytest.mark.parametrize("nq", [1, 31, 32, 33, 48])
@pytest.mark.parametrize("nt", [1, 7, 130])
def test_tile_shapes(engine, checker, nq, nt):
    rng = np.random.default_rng(nq * 1000 + nt)
    targets = [_rand(rng, int(n), b"ACGT") for n in rng.integers(100, 300, size=nt)]
    queries = []
    for i, n in enumerate(rng.integers(20, 41, size=nq)):
        t = targets[i % nt]
        cut = t[5:5 + int(n)]
        queries.append(cut if i % 3 == 0 else reverse_complement(cut) if i % 3 == 1 else _rand(rng, int(n), b"ACGT"))
    m, s, _, st, _, _ = check_both(engine, queries, targets, "HW", -1)
    assert st["path"] & 8
    assert (s["cellStrand"] & 1).any() or nq == 1


# ---- 2. every word count and mode

@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_every_word_count_and_mode(engine, checker, mode):
    rng = np.random.default_rng(200 + ["NW", "SHW", "HW"].index(mode))
    queries, targets = _planted(rng)
    seen = {"forward": False, "reverse": False, "both": False, "neither": False}
    for k in (-1, 0, 3, 20):
        m, s, best, st, fwd, rev = check_both(engine, queries, targets, mode, k)
        assert st["path"] & 8, st
        for kind, there in _kinds(fwd, rev).items():
            seen[kind] = seen[kind] or there
        if mode == "NW" and k >= 0:
            p = engine.CrossBatch(queries, targets, mode=mode, k=k)
            try:
                plain = p.run()
            finally:
                p.close()
            assert plain["word_steps"] > 0 and st["word_steps"] == 2 * plain["word_steps"], (st, plain)
        if k >= 0:
            check_hits_equal_dense(engine, queries, targets, mode, k, m, s, best)
    assert all(seen.values()), seen


# ---- 3. ties

def _tie_inputs(rng):
    half = _rand(rng, 12, b"ACGT")
    palindromes = [b"ACGT", b"GAATTC", half + reverse_complement(half)]
    base = [_rand(rng, 24, b"ACGT") for _ in range(6)]
    queries = palindromes + base + base[:3] + [reverse_complement(base[0]), reverse_complement(base[4])] + [palindromes[1]]
    targets = [_rand(rng, 150, b"ACGT") for _ in range(12)]
    for i in range(4):                               # the base queries occur, on either strand
        t = bytearray(targets[i])
        t[20:44] = base[i] if i % 2 == 0 else reverse_complement(base[i])
        t[80:86] = b"GAATTC"
        targets[i] = bytes(t)
    targets += targets[:3]
    return queries, targets, len(palindromes)


@pytest.mark.parametrize("mode,k", [("HW", -1), ("HW", 0), ("HW", 3), ("HW", 4), ("HW", 20), ("NW", 140), ("SHW", 10)])
def test_ties(engine, checker, mode, k):
    queries, targets, npal = _tie_inputs(np.random.default_rng(7))
    m, s, best, st, fwd, rev = check_both(engine, queries, targets, mode, k, runs=2)
    df, dr = fwd["editDistance"], rev["editDistance"]
    both = (s["cellStrand"] & 2) != 0
    assert np.array_equal(both, (df >= 0) & (df == dr))          # set exactly where the two distances are equal
    assert not (s["cellStrand"][both] & 1).any()                 # and then the forward fields are reported
    for f in FIELDS:
        assert np.array_equal(m[f][both], fwd[f][both]), f
    pal = s["cellStrand"][:, :npal]
    assert np.all((pal == 2) | ((pal == 0) & (m["editDistance"][:, :npal] == -1)))     # a palindrome ties everywhere
    # duplicates and a query beside its own reverse complement tie in distance: the lowest query index is the best
    ed = m["editDistance"]
    for t in range(len(targets)):
        if best["bestQuery"][t] >= 0:
            assert best["bestQuery"][t] == int(np.nonzero(ed[t] == best["bestQueryDistance"][t])[0][0])
    if k >= 0:
        check_hits_equal_dense(engine, queries, targets, mode, k, m, s, best, runs=2)


# ---- 4. alphabets

SIXTEEN = b"ACGTEFIJLNOPQSWX"          # closed under complement; all but A, C, G, T are their own complement


@pytest.mark.parametrize("alpha", ["ACGTN", "IUPAC", "lower", "16"])
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_alphabets(engine, checker, mode, alpha):
    chars, eqs, lower = {"ACGTN": (b"ACGTN", None, False), "IUPAC": (b"ACGTRYN", IUPAC, False),
                         "lower": (b"ACGT", None, True), "16": (SIXTEEN, None, False)}[alpha]
    rng = np.random.default_rng(400 + sorted(["ACGTN", "IUPAC", "lower", "16"]).index(alpha))
    queries, targets = _planted(rng, chars, nq=24, nt=40, tmax=400, lower=lower)
    seen = {"forward": False, "reverse": False, "both": False, "neither": False}
    for k in (-1, 0, 3, 20):
        m, s, best, st, fwd, rev = check_both(engine, queries, targets, mode, k, eqs)
        assert st["path"] & 8, st
        for kind, there in _kinds(fwd, rev).items():
            seen[kind] = seen[kind] or there
        if mode == "NW" and k >= 0:
            p = engine.CrossBatch(queries, targets, mode=mode, k=k, additionalEqualities=eqs)
            try:
                plain = p.run()
            finally:
                p.close()
            assert plain["word_steps"] > 0 and st["word_steps"] == 2 * plain["word_steps"], (st, plain)
    assert all(seen.values()), seen


# ---- 5. out of the kernel's envelope

def test_out_of_envelope(engine, checker):
    rng = np.random.default_rng(5)
    big = _rand(rng, 100_000, b"ACGT")
    targets = [_rand(rng, int(n), b"ACGT") for n in rng.integers(320, 500, size=6)]
    targets.insert(2, big)
    queries = [targets[0][10:310], reverse_complement(targets[1][5:305])]               # 300 bases: the pair route
    queries += [big[50_000:50_100], reverse_complement(big[70_000:70_080]), targets[3][20:90],
                reverse_complement(targets[4][20:90]), _rand(rng, 40, b"ACGT"), b""]
    for mode, k in (("HW", 12), ("NW", 250), ("HW", -1)):
        m, s, best, st, fwd, rev = check_both(engine, queries, targets, mode, k)
        assert st["path"] & 8, st
        if mode == "HW":
            assert m["editDistance"][2, 2] == 0 and s["cellStrand"][2, 2] == 0          # the shared-target sessions
            assert m["editDistance"][2, 3] == 0 and s["cellStrand"][2, 3] == 1
            assert m["editDistance"][0, 0] == 0 and s["cellStrand"][0, 0] == 0          # the pair session
            assert m["editDistance"][1, 1] == 0 and s["cellStrand"][1, 1] == 1
        if k >= 0:
            check_hits_equal_dense(engine, queries, targets, mode, k, m, s, best)


def test_wide_alphabet_routes_away_from_the_kernel(engine, checker):
    rng = np.random.default_rng(6)
    prot = b"ACDEFGHIKLMNPQRSTVWY"
    targets = [_rand(rng, int(n), prot) for n in rng.integers(0, 300, size=7)]
    queries = [_rand(rng, int(n), prot) for n in rng.integers(0, 100, size=8)]
    queries += [targets[3][5:60], reverse_complement(targets[4][5:60]), _rand(rng, 300, prot)]
    for mode, k in (("HW", -1), ("HW", 25), ("NW", 120), ("SHW", 40)):
        m, s, best, st, fwd, rev = check_both(engine, queries, targets, mode, k)
        assert not (st["path"] & 8), st               # every target through the internal both-strand sessions
        if k >= 0:
            check_hits_equal_dense(engine, queries, targets, mode, k, m, s, best)
    assert (s["cellStrand"] & 1).any()


# ---- 7. hits growth

def test_hits_growth(engine):
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qs = rng.choice(acgt, size=(1100, 8)).astype(np.uint8)
    ts = rng.choice(acgt, size=(1000, 8)).astype(np.uint8)
    b = engine.CrossBatch(qs, ts, mode="HW", k=8, hits=True, strands="both")     # every cell within k: 1.1M hits > 2^20
    d = engine.CrossBatch(qs, ts, mode="HW", k=8, strands="both")
    try:
        d.run()
        m, ds = d.matrix(), d.strands()
        launches = []
        for _ in range(2):
            st = b.run()
            launches.append(st["scan_launches"])
            h, hs = b.hits(), b.strands()
            assert len(h["query"]) == 1_100_000
            assert np.array_equal(h["targetOffsets"], np.arange(1001, dtype=np.int64) * 1100)
            assert np.array_equal(h["query"], np.tile(np.arange(1100, dtype=np.int32), 1000))
            assert np.array_equal(h["editDistance"], m["editDistance"].reshape(-1))
            assert np.array_equal(hs["hitStrand"], ds["cellStrand"].reshape(-1))
        assert launches[0] == 2 * launches[1], launches      # the first Run grew the list and scanned again, the second fits
    finally:
        b.close()
        d.close()


# ---- 8. wrong views

def test_wrong_views(engine):
    L = engine.lib()
    v = engine.CrossStrands()
    qs, ts = [b"ACGT", b"GGA"], [b"ACGTACGT", b"TCC", b""]
    both = engine.CrossBatch(qs, ts, mode="HW", strands="both")
    assert L.edlibAmdBatchCrossStrands(both._h, engine.CROSS_BEST, C.byref(v)) != 0        # before the first Run
    assert "Run" in engine.last_error()
    both.run()
    assert L.edlibAmdBatchCrossStrands(both._h, engine.CROSS_BEST, C.byref(v)) == 0
    assert not v.cellStrand and not v.hitStrand and v.bestQueryStrand and v.bestTargetStrand
    assert L.edlibAmdBatchCrossStrands(both._h, 4, C.byref(v)) != 0
    sv = engine.StrandView()
    assert L.edlibAmdBatchStrandView(both._h, C.byref(sv)) != 0
    assert "edlibAmdBatchCrossStrands" in engine.last_error()
    assert L.edlibAmdBatchResultsView(both._h, C.byref(engine.ResultsView())) != 0
    assert L.edlibAmdBatchWindowView(both._h, 1, C.byref(engine.WindowView())) != 0
    assert both.strands()["cellStrand"][1, 1] == 1 and both.matrix()["editDistance"][1, 1] == 0   # revcomp(GGA) = TCC
    hits = engine.CrossBatch(qs, ts, mode="HW", k=1, hits=True, strands="both")
    hits.run()
    assert L.edlibAmdBatchStrandView(hits._h, C.byref(sv)) != 0
    assert "edlibAmdBatchCrossStrands" in engine.last_error()
    assert L.edlibAmdBatchCrossStrands(hits._h, engine.CROSS_MATRIX, C.byref(v)) == 0
    assert v.hitStrand and not v.cellStrand and v.numHits == len(hits.hits()["query"])
    hits.close()
    both.close()
    plain = engine.CrossBatch(qs, ts, mode="HW")
    window = engine.WindowBatch(qs, b"ACGTACGT", [0], [0], [8])
    shared = engine.SharedBatch(qs, b"ACGTACGT")
    for b in (plain, window, shared):
        b.run()
        assert L.edlibAmdBatchCrossStrands(b._h, engine.CROSS_BEST, C.byref(v)) != 0
        assert engine.last_error()
        b.close()
    with pytest.raises(RuntimeError, match="strands='both'"):
        plain.strands()
    d = engine.align_cross(qs, ts, mode="HW", strands="both")
    assert d["editDistance"].shape == (3, 2) and d["cellStrand"].shape == (3, 2) and d["editDistance"][1, 1] == 0


def test_strands_without_the_cells(engine):
    """strands(cells=False) asks for the best strands alone: the same two arrays, and no cellStrand / hitStrand."""
    rng = np.random.default_rng(9)
    targets = [_rand(rng, 60, b"ACGT") for _ in range(9)]
    queries = [targets[0][5:25], reverse_complement(targets[1][5:25]), _rand(rng, 20, b"ACGT")]
    for hits in (False, True):
        b = engine.CrossBatch(queries, targets, mode="HW", k=2, hits=hits, strands="both")
        try:
            b.run()
            full, few = b.strands(), b.strands(cells=False)
        finally:
            b.close()
        assert sorted(few) == ["bestQueryStrand", "bestTargetStrand"]
        assert ("hitStrand" if hits else "cellStrand") in full
        for f in few:
            assert few[f].dtype == np.uint8 and np.array_equal(few[f], full[f]), f
        assert few["bestQueryStrand"][0] == 0 and few["bestQueryStrand"][1] == 1
