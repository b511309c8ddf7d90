"""GPU: window batches (edlibAmdBatchCreateWindows: units = a query against a window of one resident target).  Every unit
checked is compared with the checker (the compiled reference where it travelled) on the sliced bytes of its window, and
best() with window_best_model() of the units() arrays."""
import ctypes as C

import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth, window_best_model
from oracle import oracle as O

pytestmark = pytest.mark.gpu

IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]
FIELDS = ("editDistance", "numLocations", "endLocation")


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8), off


def _bytes(s):
    return s if isinstance(s, bytes) else np.asarray(s, dtype=np.uint8).tobytes()


def ref_units(queries, target, uq, us, ul, mode, k, eqs=None, sel=None):
    """(editDistance, numLocations, first end) of the units `sel` (all of them: None) by the checker, each on the bytes
    of its window."""
    idx = range(len(uq)) if sel is None else sel
    tb = _bytes(target)
    qp, qo = _pack([_bytes(queries[int(uq[u])]) for u in idx])
    tp, to = _pack([tb[int(us[u]):int(us[u]) + int(ul[u])] for u in idx])
    r = O.pool_align(qp, qo, tp, to, False, mode, "distance", k, eq_pairs=eqs)
    ed, nloc, loc, ends = (np.asarray(r[f]) for f in ("editDistance", "numLocations", "locOff", "ends"))
    first = np.where(nloc > 0, ends[np.minimum(loc[:-1], max(len(ends) - 1, 0))] if len(ends) else -1, -1)
    return {"editDistance": ed, "numLocations": nloc, "endLocation": first}


def host_word_steps(queries, uq, ul, mode, k):
    total = 0
    for q, n in zip(uq, ul):
        m = len(queries[int(q)])
        if m == 0 or n == 0 or (mode == "NW" and k >= 0 and abs(m - int(n)) > k):
            continue
        total += ((m + 31) // 32) * int(n)
    return total


def check(b, queries, target, uq, us, ul, mode, k, eqs=None, sel=None):
    """units() against the checker, best() against the model, cells against the lengths; returns (units, best)."""
    got = b.units()
    nu = len(uq)
    for f in FIELDS:
        assert got[f].shape == (nu,) and got[f].dtype == np.int32, f
    idx = np.arange(nu) if sel is None else np.asarray(sel)
    if len(idx):
        want = ref_units(queries, target, uq, us, ul, mode, k, eqs, None if sel is None else idx)
        for f in FIELDS:
            bad = np.nonzero(got[f][idx] != want[f])[0]
            assert len(bad) == 0, (f, mode, k, [(int(idx[i]), int(got[f][idx[i]]), int(want[f][i]),
                                                 len(queries[int(uq[idx[i]])]), int(us[idx[i]]), int(ul[idx[i]]))
                                                for i in bad[:5]])
    best = b.best()
    model = window_best_model(uq, got["editDistance"], len(queries))
    for f, v in model.items():
        assert best[f].dtype == np.int32 and np.array_equal(best[f], v), (f, np.nonzero(best[f] != v)[0][:5])
    assert b.stats()["cells"] == sum(len(queries[int(q)]) * int(n) for q, n in zip(uq, ul))
    return got, best


_NEXT = np.arange(256, dtype=np.uint8)
_NEXT[list(b"ACGT")] = list(b"CGTA")


def _read_from(target, pos, m, rng, edits=2):
    """m bases of the target at pos with a few substitutions."""
    r = np.array(target[pos:pos + m], dtype=np.uint8)
    at = rng.integers(0, max(m, 1), size=min(edits, m))
    r[at] = _NEXT[r[at]]
    return r.tobytes()


# ---- 1. alignment of the 4-bit fetch

@pytest.mark.parametrize("tlen", [3000, 3003])
def test_every_start_phase_and_short_length(engine, checker, tlen):
    target = synth.random_dna(101, tlen)
    rng = np.random.default_rng(tlen)
    query = _read_from(target, 1000, 100, rng, 3)
    lengths = [0, 1, 7, 8, 9, 15, 16, 17, 400]
    us, ul = [], []
    for r in range(8):
        for n in lengths:
            us.append(984 + r if n == 400 else 8 * int(rng.integers(0, (tlen - 420) // 8)) + r)
            ul.append(n)
    for n in lengths:                                   # windows that end exactly at the target's last column
        us.append(tlen - n); ul.append(n)
    assert sorted(set(s % 8 for s in us)) == list(range(8)) and tlen in [s + n for s, n in zip(us, ul)]
    uq = [0] * len(us)
    for mode in ("HW", "SHW", "NW"):
        b = engine.WindowBatch([query], target, uq, us, ul, mode=mode, k=-1)
        try:
            st = b.run()
            assert st["path"] & 16 and not st["path"] & 2, st
            check(b, [query], target, uq, us, ul, mode, -1)
        finally:
            b.close()


# ---- 2. every word count

@pytest.mark.parametrize("k", [-1, 3])
@pytest.mark.parametrize("mode", ["HW", "NW"])
def test_every_word_count(engine, checker, mode, k):
    target = synth.random_dna(102, 8000)
    rng = np.random.default_rng(7)
    queries, uq, us, ul = [], [], [], []
    for i, m in enumerate([1, 31, 32, 33, 64, 65, 128, 255, 256]):
        pos = int(rng.integers(0, 7000))
        queries.append(_read_from(target, pos, m, rng, 2))
        for n in (m, m + 1, 2 * m + 50):
            uq.append(i); us.append(pos); ul.append(n)
    b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k)
    try:
        st = b.run()
        assert st["path"] & 16 and not st["path"] & 2, st
        got, _ = check(b, queries, target, uq, us, ul, mode, k)
        assert (got["editDistance"] >= 0).any()
        assert st["word_steps"] == host_word_steps(queries, uq, ul, mode, k), st
        if mode == "NW" and k == 3:
            inside = [(q, n) for q, n in zip(uq, ul) if abs(len(queries[q]) - n) <= 3]
            assert 0 < len(inside) < len(uq)
            assert st["word_steps"] == sum(((len(queries[q]) + 31) // 32) * n for q, n in inside)
    finally:
        b.close()


# ---- 3. ragged waves

@pytest.mark.parametrize("nu", [1, 63, 64, 65, 130])
def test_ragged_waves(engine, checker, nu):
    target = synth.random_dna(103, 5000)
    rng = np.random.default_rng(nu)
    queries = [_read_from(target, int(rng.integers(0, 4000)), int(m), rng, 3) for m in rng.integers(20, 151, size=12)]
    assert len(set((len(q) + 31) // 32 for q in queries)) >= 3
    uq = rng.integers(0, len(queries), size=nu)
    ul = rng.integers(1, 601, size=nu)
    us = np.array([rng.integers(0, 5000 - n + 1) for n in ul])
    b = engine.WindowBatch(queries, target, uq, us, ul, mode="HW")
    try:
        st = b.run()
        assert st["path"] & 16 and not st["path"] & 2, st
        assert st["word_steps"] == host_word_steps(queries, uq, ul, "HW", -1), st
        check(b, queries, target, uq, us, ul, "HW", -1)
    finally:
        b.close()


# ---- 4. unit list shapes

def test_unit_list_shapes(engine, checker):
    target = synth.random_dna(104, 4000)
    rng = np.random.default_rng(4)
    q0 = bytes(target[2000:2060])                       # an exact copy: distance 0 in every window that holds it
    q1 = _read_from(target, 100, 80, rng, 1)            # named by no unit
    q2 = synth.random_dna(105, 100).tobytes()           # unrelated to every window: above k = 1
    queries = [q0, q1, q2]
    uq, us, ul = [], [], []
    for i in range(200):                                # query 0: identical, overlapping and unrelated windows
        if i in (5, 17, 90):
            s, n = 1990, 100
        elif i % 3 == 0:
            s, n = 1950 + i // 3, 150                   # overlapping windows around the locus
        else:
            s, n = int(rng.integers(0, 3800)), int(rng.integers(60, 200))
        uq.append(0); us.append(s); ul.append(n)
    for i in range(20):
        uq.append(2); us.append(int(rng.integers(0, 3700))); ul.append(300)
    k = 1
    b = engine.WindowBatch(queries, target, uq, us, ul, mode="HW", k=k)
    try:
        b.run()
        got, best = check(b, queries, target, uq, us, ul, "HW", k)
        first = {f: got[f].copy() for f in FIELDS}
        best1 = {f: v.copy() for f, v in best.items()}
        ed = got["editDistance"]
        zero = np.nonzero(ed[:200] == 0)[0]
        assert len(zero) >= 4 and ed[5] == ed[17] == ed[90] == 0
        assert best["bestUnit"][0] == zero[0] and best["bestDistance"][0] == 0 and best["secondDistance"][0] == 0
        assert best["bestUnit"][1] == best["bestDistance"][1] == best["secondDistance"][1] == -1
        assert (ed[200:] == -1).all()
        assert best["bestUnit"][2] == best["bestDistance"][2] == best["secondDistance"][2] == -1
        b.run()                                         # a second Run: the same views
        again, best2 = b.units(), b.best()
        for f in FIELDS:
            assert np.array_equal(again[f], first[f]), f
        for f in best1:
            assert np.array_equal(best2[f], best1[f]), f
    finally:
        b.close()


def test_no_units(engine):
    b = engine.WindowBatch([b"ACGT", b""], synth.random_dna(106, 3000), [], [], [], mode="HW")
    try:
        st = b.run()
        assert st["cells"] == 0 and st["word_steps"] == 0 and not st["path"] & 18, st
        u, best = b.units(), b.best()
        for f in FIELDS:
            assert u[f].shape == (0,)
        for f in ("bestUnit", "bestDistance", "secondDistance"):
            assert np.array_equal(best[f], [-1, -1]), f
    finally:
        b.close()


# ---- 5. alphabets

def _alphabet_case(engine, target, eqs, seed, mode="HW", k=-1):
    rng = np.random.default_rng(seed)
    n = 300
    starts = rng.integers(0, len(target) - 500, size=40)
    queries = []
    for s in starts:
        q = np.array(target[s + 50:s + 50 + int(rng.integers(30, 200))], dtype=np.uint8)
        q[rng.integers(0, len(q), size=2)] = ord("A")
        queries.append(q.tobytes())
    uq = rng.integers(0, len(queries), size=n)
    ul = rng.integers(1, 450, size=n)
    us = np.where(np.arange(n) % 2 == 0, starts[uq], rng.integers(0, len(target) - 500, size=n))   # half at their locus
    b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k, additionalEqualities=eqs)
    try:
        st = b.run()
        check(b, queries, target, uq, us, ul, mode, k, eqs)
        return st
    finally:
        b.close()


def test_five_symbol_target(engine, checker):
    target = synth.masked_genome(41, 12000, frac_n=0.03, frac_lower=0.0)
    assert 5 <= len(set(target.tolist())) <= 8
    st = _alphabet_case(engine, target, None, 51)
    assert st["path"] & 16 and not st["path"] & 2, st


def test_nine_symbol_target(engine, checker):
    target = synth.masked_genome(43, 12000, frac_n=0.03, frac_lower=0.2)
    assert 9 <= len(set(target.tolist())) <= 16
    st = _alphabet_case(engine, target, None, 52, mode="SHW", k=40)
    assert st["path"] & 16 and not st["path"] & 2, st


def test_iupac_equalities(engine, checker):
    target = synth.masked_genome(43, 12000, frac_n=0.03, iupac=True)
    assert 9 <= len(set(target.tolist())) <= 16
    st = _alphabet_case(engine, target, IUPAC, 53)
    assert st["path"] & 16 and not st["path"] & 2, st


def test_seventeen_symbols_take_the_pair_batch(engine, checker):
    target = synth.random_symbols(44, 6000, 17)
    assert len(set(target.tolist())) == 17
    st = _alphabet_case(engine, target, None, 54)
    assert st["path"] & 2 and not st["path"] & 16, st


# ---- 6. mixed envelope

@pytest.mark.parametrize("mode", ["HW", "NW", "SHW"])
def test_mixed_envelope(engine, checker, mode):
    target = synth.random_dna(107, 6000)
    rng = np.random.default_rng(6)
    queries = [_read_from(target, 500, 257, rng, 4), _read_from(target, 1500, 600, rng, 6), b"",
               _read_from(target, 3000, 150, rng, 2), _read_from(target, 4000, 40, rng, 1)]
    units = [(0, 480, 300), (0, 500, 257), (1, 1450, 700), (1, 1500, 600), (2, 100, 50), (2, 200, 0),
             (3, 2950, 400), (3, 3000, 150), (3, 17, 0), (4, 4000, 40), (4, 3990, 90), (0, 5000, 0), (3, 5600, 400)]
    units += [(int(rng.integers(3, 5)), int(rng.integers(0, 5000)), int(rng.integers(1, 500))) for _ in range(100)]
    uq, us, ul = (np.array(x) for x in zip(*units))
    for k in (-1, 10):
        b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k)
        try:
            st = b.run()
            assert st["path"] & 16 and st["path"] & 2, st
            if mode == "HW" and k == -1:
                # word_steps: the kernel's units, and the internal pair session's own count (the same session made here)
                out = np.array([len(queries[int(q)]) > 256 for q in uq])
                tb = _bytes(target)
                p = engine.PairBatch([queries[int(q)] for q in uq[out]],
                                     [tb[int(s):int(s) + int(n)] for s, n in zip(us[out], ul[out])], mode=mode, k=k)
                try:
                    pair_steps = p.run()["word_steps"]
                finally:
                    p.close()
                kernel = host_word_steps(queries, uq[~out], ul[~out], mode, k)
                print("word_steps", st["word_steps"], kernel, pair_steps)
                assert st["word_steps"] == kernel + pair_steps, (st["word_steps"], kernel, pair_steps)
            check(b, queries, target, uq, us, ul, mode, k)
        finally:
            b.close()


# ---- 7. against the product's other route, larger

def test_reads_with_four_candidates(engine, checker):
    nreads, m, w = 5000, 150, 400
    target = synth.random_dna(108, 200_000)
    R = synth.illumina_reads(target, nreads, m=m, seed=109)
    reads, pos = R["reads"], np.asarray(R["start"], dtype=np.int64)
    rng = np.random.default_rng(8)
    true_start = np.clip(pos - 125, 0, len(target) - w)
    us = rng.integers(0, len(target) - w + 1, size=(nreads, 4))
    slot = rng.integers(0, 4, size=nreads)              # where among its four the true locus sits
    us[np.arange(nreads), slot] = true_start
    us = us.reshape(-1)
    uq = np.repeat(np.arange(nreads), 4)
    ul = np.full(4 * nreads, w)
    b = engine.WindowBatch(reads, target, uq, us, ul, mode="HW")
    try:
        st = b.run()
        assert st["path"] & 16 and not st["path"] & 2, st
        assert st["word_steps"] == 4 * nreads * 5 * w
        got, best = check(b, reads, target, uq, us, ul, "HW", -1, sel=np.arange(0, 4 * nreads, 40))
    finally:
        b.close()
    wins = np.ascontiguousarray(target[us[:, None] + np.arange(w)[None, :]])
    p = engine.PairBatch(np.ascontiguousarray(reads[uq]), wins, mode="HW", task="distance")
    try:
        p.run()
        f = p.results_flat()
    finally:
        p.close()
    assert np.array_equal(got["editDistance"], f["editDistance"])
    assert np.array_equal(got["numLocations"], f["numLocations"])
    assert (f["numLocations"] > 0).all()
    assert np.array_equal(got["endLocation"], f["ends"][f["locOff"][:-1]])
    ed4 = got["editDistance"].reshape(nreads, 4)
    true_ed = ed4[np.arange(nreads), slot]
    others = np.where(np.arange(4)[None, :] == slot[:, None], np.iinfo(np.int32).max, ed4).min(axis=1)
    clear = true_ed < others
    assert clear.sum() > nreads // 2
    assert np.array_equal(best["bestUnit"][clear], (4 * np.arange(nreads) + slot)[clear])


# ---- 8. wrong views

def _views(L, h):
    """The eight views of the other batch kinds, each as (name, status) on handle h."""
    n = 4
    res = (edlib_amd.AlignResult * n)()
    ints = [(C.c_int * n)() for _ in range(4)]
    offs = [(C.c_longlong * (n + 1))() for _ in range(2)]
    ptrs = [C.c_void_p() for _ in range(3)]
    pc, po = C.c_void_p(), C.c_void_p()
    calls = [
        ("Results", lambda: L.edlibAmdBatchResults(h, res)),
        ("ResultsFlat", lambda: L.edlibAmdBatchResultsFlat(h, ints[0], ints[1], ints[2], ints[3], offs[0], C.byref(ptrs[0]),
                                                           C.byref(ptrs[1]), offs[1], C.byref(ptrs[2]))),
        ("ResultsView", lambda: L.edlibAmdBatchResultsView(h, C.byref(edlib_amd.ResultsView()))),
        ("CigarView", lambda: L.edlibAmdBatchCigarView(h, 1, C.byref(pc), C.byref(po))),
        ("StrandView", lambda: L.edlibAmdBatchStrandView(h, C.byref(edlib_amd.StrandView()))),
        ("CrossView", lambda: L.edlibAmdBatchCrossView(h, edlib_amd.CROSS_BEST, C.byref(edlib_amd.CrossView()))),
        ("CrossHits", lambda: L.edlibAmdBatchCrossHits(h, C.byref(edlib_amd.CrossHits()))),
        ("SharedHits", lambda: L.edlibAmdBatchSharedHits(h, C.byref(edlib_amd.ReadHits()))),
    ]
    return [(name, f(), edlib_amd.last_error()) for name, f in calls]


def test_wrong_views(engine):
    L = engine.lib()
    target = synth.random_dna(110, 3000)
    reads = [bytes(target[100:150]), bytes(target[900:1000])]
    b = engine.WindowBatch(reads, target, [0, 1, 1, 0], [90, 880, 0, 2000], [80, 150, 100, 60], mode="HW")
    try:
        v = edlib_amd.WindowView()
        assert L.edlibAmdBatchWindowView(b._h, edlib_amd.WINDOW_UNITS, C.byref(v)) != 0       # before the first Run
        assert "Run" in engine.last_error()
        with pytest.raises(RuntimeError):
            b.units()
        b.run()
        for name, status, err in _views(L, b._h):
            assert status != 0, name
            assert "window batch" in err, (name, err)
        with pytest.raises(RuntimeError, match="window batch"):
            b.results()
        assert L.edlibAmdBatchWindowView(b._h, 4, C.byref(v)) != 0                            # an unknown part
        assert L.edlibAmdBatchWindowView(b._h, edlib_amd.WINDOW_BEST, C.byref(v)) == 0
        assert v.numUnits == 4 and v.numQueries == 2 and not v.editDistance and v.bestUnit    # only the parts asked for
        assert [v.bestUnit[i] for i in range(2)] == [0, 1]
    finally:
        b.close()
    others = [engine.SharedBatch(reads, target, mode="HW"), engine.PairBatch(reads, [target, target], mode="HW"),
              engine.CrossBatch(reads, [target], mode="HW")]
    try:
        for o in others:
            o.run()
            v = edlib_amd.WindowView()
            assert L.edlibAmdBatchWindowView(o._h, edlib_amd.WINDOW_UNITS, C.byref(v)) != 0, type(o).__name__
            assert "not a window batch" in engine.last_error()
    finally:
        for o in others:
            o.close()
