"""GPU: cross batches (edlibAmdBatchCreateCross, every query against every target).  Every cell checked is compared with
the checker (the compiled reference where it travelled) over the expanded pairs; best hits with a numpy reduction of the
matrix."""
import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth
from oracle import oracle as O
from test_cross_api import best_model

pytestmark = pytest.mark.gpu

IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]


def _rand(rng, n, alpha):
    return bytes(rng.choice(np.frombuffer(alpha, dtype=np.uint8), size=n).astype(np.uint8))


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8), off


def ref_cells(queries, targets, mode, k, eqs, tq):
    """(editDistance, numLocations, first end) of the cells tq = [(t, q)] by the checker."""
    qs = [queries[q] for t, q in tq]
    ts = [targets[t] for t, q in tq]
    qp, qo = _pack(qs)
    tp, to = _pack(ts)
    r = O.pool_align(qp, qo, tp, to, False, mode, "distance", k, eq_pairs=eqs)
    ed = np.asarray(r["editDistance"])
    nloc = np.asarray(r["numLocations"])
    loc = np.asarray(r["locOff"])
    ends = np.asarray(r["ends"])
    first = np.where(nloc > 0, ends[np.minimum(loc[:-1], max(len(ends) - 1, 0))] if len(ends) else -1, -1)
    return ed, nloc, first


def check_cells(b, queries, targets, mode, k, eqs=None, sample=None, seed=0):
    m = b.matrix()
    nt, nq = len(targets), len(queries)
    assert m["editDistance"].shape == (nt, nq)
    if sample is None or sample >= nt * nq:
        tq = [(t, q) for t in range(nt) for q in range(nq)]
    else:
        rng = np.random.default_rng(seed)
        idx = rng.choice(nt * nq, size=sample, replace=False)
        tq = [(int(i) // nq, int(i) % nq) for i in idx]
    if not tq:
        return m
    ed, nloc, first = ref_cells(queries, targets, mode, k, eqs, tq)
    t_ = np.array([a for a, _ in tq]); q_ = np.array([c for _, c in tq])
    for name, want in (("editDistance", ed), ("numLocations", nloc), ("endLocation", first)):
        got = m[name][t_, q_]
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, mode, k, [(tq[i], int(got[i]), int(want[i]), len(queries[tq[i][1]]), len(targets[tq[i][0]]))
                                                for i in bad[:5]])
    return m


def check_best(b, m=None):
    if m is None:
        m = b.matrix()
    got = b.best()
    want = best_model(m["editDistance"])
    for f, v in want.items():
        assert np.array_equal(got[f], v), (f, np.nonzero(got[f] != v)[0][:5])
    return got


def _mixed(rng, alpha, nq=100, nt=300):
    qlens = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256] + list(rng.integers(1, 257, size=nq - 11)) + [0]
    tlens = [0, 1, 2000] + list(rng.integers(1, 2001, size=nt - 4)) + [0]
    targets = [_rand(rng, int(n), alpha) for n in tlens]
    queries = []
    for i, n in enumerate(qlens):
        if i % 3 == 0 and n > 0:               # a query taken from a target (small distances somewhere)
            t = targets[2]
            s = int(rng.integers(0, len(t) - n + 1))
            queries.append(t[s:s + n])
        else:
            queries.append(_rand(rng, int(n), alpha))
    return queries, targets


ALPHABETS = {"ACGT": (b"ACGT", None), "ACGTN": (b"ACGTN", None), "IUPAC": (b"ACGTRYN", IUPAC),
             "16": (b"ACDEFGHIKLMNPQRS", None)}


@pytest.mark.parametrize("alpha", sorted(ALPHABETS))
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_cross_cells_match_reference(engine, checker, mode, alpha):
    chars, eqs = ALPHABETS[alpha]
    rng = np.random.default_rng(hash((mode, alpha)) & 0xffff)
    queries, targets = _mixed(rng, chars)
    for k in (-1, 0, 3, 20):
        b = engine.CrossBatch(queries, targets, mode=mode, k=k, additionalEqualities=eqs)
        try:
            st = b.run()
            assert st["path"] & 8, st
            assert st["cells"] == sum(map(len, queries)) * sum(map(len, targets))
            m = check_cells(b, queries, targets, mode, k, eqs)
            check_best(b, m)
        finally:
            b.close()


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 96])
@pytest.mark.parametrize("nt", [1, 7, 130])
def test_cross_tile_shapes(engine, checker, nq, nt):
    rng = np.random.default_rng(nq * 1000 + nt)
    queries = [_rand(rng, int(n), b"ACGT") for n in rng.integers(20, 41, size=nq)]
    targets = [_rand(rng, int(n), b"ACGT") for n in rng.integers(100, 300, size=nt)]
    b = engine.CrossBatch(queries, targets, mode="HW")
    b.run()
    m = check_cells(b, queries, targets, "HW", -1)
    check_best(b, m)
    b.close()


def test_cross_out_of_envelope(engine, checker):
    rng = np.random.default_rng(5)
    # a 300-base query (pair route) and a 1 Mb target (shared-target route) among short ones
    queries = [_rand(rng, 300, b"ACGT")] + [_rand(rng, int(n), b"ACGT") for n in rng.integers(20, 200, size=20)]
    big = synth.random_dna(11, 1_000_000)
    big = big.tobytes() if hasattr(big, "tobytes") else bytes(big)
    targets = [_rand(rng, int(n), b"ACGT") for n in rng.integers(50, 500, size=30)]
    targets.insert(7, big)
    queries.append(big[500_000:500_120])
    for mode in ("HW", "NW"):
        b = engine.CrossBatch(queries, targets, mode=mode, k=-1 if mode == "HW" else 200)
        st = b.run()
        assert st["path"] & 8
        if mode == "HW":
            # word_steps: the kernel's cells, and the internal sessions' own counts (the same sessions made here)
            small = sorted((t for t in range(len(targets)) if t != 7), key=lambda t: len(targets[t]))
            kernel = sum((len(q) + 31) // 32 for q in queries if len(q) <= 256) * sum(len(targets[t]) for t in small)
            parts = [kernel]
            for s in (engine.SharedBatch(queries, big, mode="HW", k=-1),
                      engine.PairBatch([queries[0]] * len(small), [targets[t] for t in small], mode="HW", k=-1)):
                try:
                    parts.append(s.run()["word_steps"])
                finally:
                    s.close()
            print("word_steps", st["word_steps"], parts)
            assert st["word_steps"] == sum(parts), (st["word_steps"], parts)
        tq = [(t, q) for t in range(len(targets)) for q in range(len(queries)) if t != 7 or q % 4 == 0 or q == len(queries) - 1]
        m = b.matrix()
        ed, nloc, first = ref_cells(queries, targets, mode, -1 if mode == "HW" else 200, None, tq)
        t_ = np.array([a for a, _ in tq]); q_ = np.array([c for _, c in tq])
        assert np.array_equal(m["editDistance"][t_, q_], ed)
        assert np.array_equal(m["numLocations"][t_, q_], nloc)
        assert np.array_equal(m["endLocation"][t_, q_], first)
        if mode == "HW":
            assert m["editDistance"][7, len(queries) - 1] == 0
        check_best(b, m)
        b.close()


def test_cross_wide_alphabet(engine, checker):
    rng = np.random.default_rng(6)
    prot = b"ACDEFGHIKLMNPQRSTVWY"
    queries = [_rand(rng, int(n), prot) for n in rng.integers(0, 120, size=12)]
    targets = [_rand(rng, int(n), prot) for n in rng.integers(0, 400, size=9)]
    for mode in ("NW", "SHW", "HW"):
        b = engine.CrossBatch(queries, targets, mode=mode, k=-1)
        st = b.run()
        assert not (st["path"] & 8)           # every target through the shared-target engine
        m = check_cells(b, queries, targets, mode, -1)
        check_best(b, m)
        b.close()


def test_cross_ties_and_repeats(engine, checker):
    rng = np.random.default_rng(7)
    base_q = [_rand(rng, 24, b"ACGT") for _ in range(10)]
    queries = base_q + base_q[:4] + [base_q[0]]
    base_t = [_rand(rng, 150, b"ACGT") for _ in range(20)]
    targets = base_t + base_t[:5]
    for mode, k in (("HW", -1), ("HW", 4), ("NW", 100), ("SHW", 10)):
        b = engine.CrossBatch(queries, targets, mode=mode, k=k)
        b.run()
        m1 = b.matrix(); b1 = b.best()
        check_cells(b, queries, targets, mode, k)
        check_best(b, m1)
        b.run()                                # two runs: identical views
        m2 = b.matrix(); b2 = b.best()
        for f in m1:
            assert np.array_equal(m1[f], m2[f])
        for f in b1:
            assert np.array_equal(b1[f], b2[f])
        b.close()


def test_cross_views_and_refusals(engine):
    L = engine.lib()
    b = engine.CrossBatch([b"ACGT", b"GGA"], [b"ACGTACGT", b"TTT", b""], mode="HW")
    b.run()
    v = b._view(engine.CROSS_BEST)
    assert not v.editDistance and not v.numLocations and not v.endLocation
    assert v.bestQuery and v.bestTarget and v.numQueries == 2 and v.numTargets == 3
    arr = (engine.AlignResult * 6)()
    assert L.edlibAmdBatchResults(b._h, arr) != 0
    assert "cross" in engine.last_error()
    rv = engine.ResultsView()
    assert L.edlibAmdBatchResultsView(b._h, engine.C.byref(rv)) != 0
    assert "cross" in engine.last_error()
    import ctypes as C
    pc, po = C.c_void_p(), C.c_void_p()
    assert L.edlibAmdBatchCigarView(b._h, 1, C.byref(pc), C.byref(po)) != 0
    assert "cross" in engine.last_error()
    assert L.edlibAmdBatchResultsFlat(b._h, *([None] * 9)) != 0
    # the other kinds of batch have no cross view
    s = engine.SharedBatch([b"ACGT"], b"ACGTACGT")
    s.run()
    cv = engine.CrossView()
    assert L.edlibAmdBatchCrossView(s._h, engine.CROSS_BEST, C.byref(cv)) != 0
    s.close()
    # one-shot form
    d = engine.align_cross([b"ACGT", b"GGA"], [b"ACGTACGT", b"TTT", b""], mode="HW")
    assert d["editDistance"].shape == (3, 2)
    assert d["editDistance"][0, 0] == 0 and d["bestQuery"][0] == 0
    b.close()


def _demux_shape(rng, nreads, nbc=96, bclen=24, rlen=150):
    barcodes = [_rand(rng, bclen, b"ACGT") for _ in range(nbc)]
    reads = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(nreads, rlen)).astype(np.uint8)
    which = rng.integers(0, nbc, size=nreads)
    for i in range(nreads):
        if i % 5:
            reads[i, 10:10 + bclen] = np.frombuffer(barcodes[which[i]], dtype=np.uint8)
            reads[i, 10 + int(rng.integers(0, bclen))] = ord("A")
    return barcodes, reads


def _check_at_size(engine, queries, targets_arr, mode, k):
    targets = [targets_arr[i].tobytes() for i in range(len(targets_arr))] if isinstance(targets_arr, np.ndarray) else targets_arr
    b = engine.CrossBatch(queries, targets_arr, mode=mode, k=k)
    b.run()
    m = check_cells(b, queries, targets, mode, k, sample=20_000, seed=3)
    check_best(b, m)
    # a 500 x 500 block against PairBatch on the same cells
    tq = [(t, q) for t in range(min(500, len(targets))) for q in range(min(500, len(queries)))]
    p = engine.PairBatch([queries[q] for _, q in tq], [targets[t] for t, _ in tq], mode=mode, k=k)
    p.run()
    f = p.results_flat()
    t_ = np.array([a for a, _ in tq]); q_ = np.array([c for _, c in tq])
    assert np.array_equal(m["editDistance"][t_, q_], f["editDistance"])
    assert np.array_equal(m["numLocations"][t_, q_], f["numLocations"])
    p.close()
    b.close()


def test_cross_demux_at_size(engine, checker):
    rng = np.random.default_rng(8)
    barcodes, reads = _demux_shape(rng, 200_000)
    _check_at_size(engine, barcodes, reads, "HW", -1)


def test_cross_all_against_all_at_size(engine, checker):
    rng = np.random.default_rng(9)
    base = _rand(rng, 150, b"ACGT")
    amp = []
    for i in range(2000):
        s = bytearray(base)
        for _ in range(int(rng.integers(0, 12))):
            s[int(rng.integers(0, 150))] = int(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8)))
        amp.append(bytes(s))
    _check_at_size(engine, amp, amp, "NW", -1)
