"""GPU: occurrence cross batches (edlibAmdBatchCreateCrossOccurrences): every maximal run of target columns within k of
every (query, target) cell, as CSR by target.  The whole view is compared field by field with the CPU model
(cross_occ_model, itself tied to the oracle in test_cross_occurrences_model.py), its order is checked on its own, and it is
held against a hit-list cross batch over the same inputs."""
import ctypes as C

import numpy as np
import pytest

import cross_occ_model as M

pytestmark = pytest.mark.gpu

LENGTHS = (1, 31, 32, 33, 64, 65, 96, 128, 129, 160, 192, 224, 255, 256)
ALPHABETS = {"ACGT": b"ACGT", "ACGTN": b"ACGTN", "12": b"ACDEFGHIKLMN"}     # S = 4 / 8 / 16
N_EQ = [("N", c) for c in "ACGT"]


def _rand(rng, n, alpha):
    return bytes(rng.choice(np.frombuffer(alpha, dtype=np.uint8), size=n).astype(np.uint8))


def _mutated(rng, s, alpha, edits):
    s = bytearray(s)
    for _ in range(edits):
        if not s:
            break
        at = int(rng.integers(0, len(s)))
        how = int(rng.integers(0, 3))
        c = int(rng.choice(np.frombuffer(alpha, dtype=np.uint8)))
        if how == 0:
            s[at] = c
        elif how == 1:
            s.insert(at, c)
        else:
            del s[at]
    return bytes(s)


def _occ_of(engine, queries, targets, k, eqs=None, runs=1):
    b = engine.CrossBatch(queries, targets, mode="HW", k=k, additionalEqualities=eqs, occurrences=True)
    try:
        out = []
        for _ in range(runs):
            st = b.run()
            out.append((b.occurrences(), st))
        return out[0] if runs == 1 else out
    finally:
        b.close()


def _planted(rng, alpha, nq=42, nt=70, cap=300):
    """queries of every word count; targets of 0 .. cap bases that carry copies of some queries (exact or with up to two
    edits): one from column 0, one flush with the last column, two back to back in between"""
    queries = [_rand(rng, n, alpha) for n in LENGTHS for _ in range(nq // len(LENGTHS))]
    targets = [b"", _rand(rng, 1, alpha), _rand(rng, cap, alpha)]
    while len(targets) < nt:
        room = cap
        def copy():
            nonlocal room
            fit = [q for q in queries if len(q) + 2 <= room]
            if not fit:
                return b""
            c = _mutated(rng, fit[int(rng.integers(0, len(fit)))], alpha, int(rng.integers(0, 3)))
            room -= len(c)
            return c
        head, tail = copy(), copy()
        pair = copy() + copy() if len(targets) % 2 else b""
        def fill():
            nonlocal room
            f = _rand(rng, int(rng.integers(0, min(room, 40) + 1)), alpha)
            room -= len(f)
            return f
        targets.append(head + fill() + pair + fill() + tail)
    return queries, targets


@pytest.mark.parametrize("alpha", sorted(ALPHABETS))
def test_word_counts_and_symbol_classes(engine, alpha):
    rng = np.random.default_rng(700 + sorted(ALPHABETS).index(alpha))
    queries, targets = _planted(rng, ALPHABETS[alpha])
    assert max(len(t) for t in targets) <= 300 and min(len(t) for t in targets) == 0
    for k in (0, 2, 256):
        occ, st = _occ_of(engine, queries, targets, k)
        assert st["path"] == 8, st
        M.assert_equal(occ, M.occurrences(queries, targets, k))
        M.assert_ordered(occ, len(queries))
        if k == 0:
            assert len(occ["query"]) > len(targets)                       # the planted exact copies are found
        if k == 256:                                                      # k >= m: one run per non-empty target
            nonEmpty = sum(1 for t in targets if t)
            assert len(occ["query"]) == nonEmpty * len(queries)
            assert np.all(occ["firstEnd"] == 0)


@pytest.mark.parametrize("n", [7, 8, 9, 15, 16, 17])
def test_target_tails(engine, n):
    """an occurrence that ends in the last column of a target whose length is (not) a multiple of the 8-column word: the
    run open at the end of the target is closed, and closed once"""
    rng = np.random.default_rng(n)
    queries = [b"ACGTA", b"GGT", b"A"]
    targets = []
    for q in queries:
        for _ in range(3):
            targets.append((_rand(rng, n, b"CT") + q)[-n:])               # q flush with the last column
    for k in (0, 1):
        occ, _ = _occ_of(engine, queries, targets, k)
        want = M.occurrences(queries, targets, k)
        M.assert_equal(occ, want)
        for t in range(len(targets)):
            runs = M.cell_runs(occ, t, t // 3)
            assert runs and runs[-1][1] == n - 1, (t, runs)
            assert sum(1 for r in runs if r[1] == n - 1) == 1


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("nq", [1, 2, 3, 64, 65])
def test_tile_shapes(engine, nq, nt):
    rng = np.random.default_rng(nq * 1000 + nt)
    queries = [_rand(rng, int(n), b"ACGT") for n in rng.integers(6, 13, size=nq)]
    targets = [_rand(rng, int(n), b"ACGT") for n in rng.integers(10, 60, size=nt)]
    for t in range(0, nt, 3):
        targets[t] = targets[t] + queries[t % nq]
    occ, st = _occ_of(engine, queries, targets, 2)
    assert st["path"] == 8
    M.assert_equal(occ, M.occurrences(queries, targets, 2))
    M.assert_ordered(occ, nq)


def test_empty_cases(engine):
    qs, ts = [b"", b"ACG", b"T", b""], [b"", b"ACGACG", b"A", b"", b"TTTTTTTTT"]
    for k in (0, 1, 3):
        occ, _ = _occ_of(engine, qs, ts, k)
        M.assert_equal(occ, M.occurrences(qs, ts, k))
    assert M.cell_runs(occ, 4, 0) == [(0, 8, 0, 0, 9)] and M.cell_runs(occ, 4, 3) == [(0, 8, 0, 0, 9)]
    assert occ["targetOffsets"][1] == 0 and occ["targetOffsets"][4] == occ["targetOffsets"][3]
    for q, t in (([], ts), (qs, []), ([], []), ([b""], [b""])):
        occ, st = _occ_of(engine, q, t, 1)
        assert len(occ["query"]) == 0 and occ["targetOffsets"].tolist() == [0] * (len(t) + 1)


def test_equalities(engine):
    rng = np.random.default_rng(9)
    queries = [_rand(rng, int(n), b"ACGTN") for n in (5, 12, 33, 40, 70)]
    targets = [_rand(rng, int(n), b"ACGTN") for n in rng.integers(0, 120, size=20)]
    targets += [queries[1].replace(b"A", b"N") + b"NNNN" + queries[3]]
    for k in (0, 2):
        occ, _ = _occ_of(engine, queries, targets, k, N_EQ)
        M.assert_equal(occ, M.occurrences(queries, targets, k, N_EQ))
        plain, _ = _occ_of(engine, queries, targets, k)
        assert len(plain["query"]) < len(occ["query"])


def test_against_hit_list_cross_batch(engine):
    rng = np.random.default_rng(11)
    queries, targets = _planted(rng, b"ACGT", nq=28, nt=50)
    for k in (0, 2, 9):
        occ, st = _occ_of(engine, queries, targets, k)
        M.assert_ordered(occ, len(queries))
        b = engine.CrossBatch(queries, targets, mode="HW", k=k, hits=True)
        try:
            hst = b.run()
            h = b.hits()
        finally:
            b.close()
        assert st["word_steps"] == hst["word_steps"] and st["cells"] == hst["cells"]
        cells, hcells = {}, {}
        for t in range(len(targets)):
            for i in range(int(occ["targetOffsets"][t]), int(occ["targetOffsets"][t + 1])):
                cells.setdefault((t, int(occ["query"][i])), []).append(
                    (int(occ["editDistance"][i]), int(occ["endLocation"][i])))
            for i in range(int(h["targetOffsets"][t]), int(h["targetOffsets"][t + 1])):
                if len(targets[t]) > 0:                                    # (the hit list reports cells of an empty target)
                    hcells[(t, int(h["query"][i]))] = (int(h["editDistance"][i]), int(h["endLocation"][i]))
        assert set(cells) == set(hcells)
        for c, runs in cells.items():
            ed, end = hcells[c]
            assert min(r[0] for r in runs) == ed, c
            if end >= 0:
                assert [r for r in runs if r[0] == ed][0][1] == end, c


def test_capacity_growth(engine):
    """1,065,600 runs against a list that starts at 2^20: the first Run counts, grows and scans again; the second fits"""
    unit, copies, nt = b"ACGTACGTCCCC", 666, 1600
    target = unit * copies + b"C" * (8000 - len(unit) * copies)
    assert len(target) == 8000
    (occ, st1), (occ2, st2) = _occ_of(engine, [b"ACGTACGT"], [target] * nt, 0, runs=2)
    assert np.array_equal(occ["targetOffsets"], np.arange(nt + 1, dtype=np.int64) * copies)      # exact per target
    assert len(occ["query"]) == 1_065_600 and not occ["query"].any()
    first = np.tile(np.arange(copies, dtype=np.int32) * 12 + 7, nt)
    for f in ("firstEnd", "lastEnd", "endLocation"):
        assert np.array_equal(occ[f], first), f
    assert not occ["editDistance"].any() and np.all(occ["numLocations"] == 1)
    assert np.array_equal(occ2["targetOffsets"], occ["targetOffsets"])
    for f in M.FIELDS:
        assert np.array_equal(occ2[f], occ[f]), f
    assert st1["scan_launches"] == 2 * st2["scan_launches"] and st2["scan_launches"] >= 1, (st1, st2)


def test_other_route(engine):
    """a target above the kernel's 65,536 columns runs through an internal hit-list session; its runs sit at its index"""
    rng = np.random.default_rng(13)
    queries = [_rand(rng, int(n), b"ACGT") for n in rng.integers(20, 65, size=30)]
    targets = [_rand(rng, int(n), b"ACGT") + queries[i] for i, n in enumerate(rng.integers(30, 200, size=5))]
    big = bytearray(_rand(rng, 70_000 - sum(len(q) for q in queries[:12]) - len(queries[3]), b"ACGT"))
    for i, q in enumerate(queries[:12]):
        at = 5000 * i + 17
        big[at:at] = _mutated(rng, q, b"ACGT", i % 3)
    big += queries[3]                                                     # flush with the last column
    assert len(big) >= 70_000 - 24
    targets.insert(2, bytes(big))
    occ, st = _occ_of(engine, queries, targets, 3)
    assert st["path"] & 8 and st["path"] & 1, st
    want = M.occurrences(queries, targets, 3)
    M.assert_equal(occ, want)
    M.assert_ordered(occ, len(queries))
    assert occ["targetOffsets"][3] - occ["targetOffsets"][2] >= 13


def _view_fails(engine, fn, handle, view, *args):
    rc = fn(handle, *args, C.byref(view))
    return (rc != 0), engine.last_error()


def test_kinds(engine):
    L = engine.lib()
    qs, ts = [b"ACGT", b"GGA"], [b"ACGTACGT", b"TTGGATT", b""]
    b = engine.CrossBatch(qs, ts, mode="HW", k=1, occurrences=True)
    dense = engine.CrossBatch(qs, ts, mode="HW", k=1)
    hits = engine.CrossBatch(qs, ts, mode="HW", k=1, hits=True)
    selfb = engine.SelfBatch([b"ACGT", b"ACGA", b"TTTT"], k=2)
    try:
        failed, err = _view_fails(engine, L.edlibAmdBatchCrossOccurrences, b._h, engine.CrossOccurrences())
        assert failed and "Run it first" in err, err
        b.run()
        first = b.occurrences()
        for fn, view, args in ((L.edlibAmdBatchCrossView, engine.CrossView(), (engine.CROSS_BEST,)),
                               (L.edlibAmdBatchCrossHits, engine.CrossHits(), ()),
                               (L.edlibAmdBatchCrossStrands, engine.CrossStrands(), (engine.CROSS_BEST,))):
            failed, err = _view_fails(engine, fn, b._h, view, *args)
            assert failed and "edlibAmdBatchCrossOccurrences" in err, err
        with pytest.raises(RuntimeError, match="edlibAmdBatchCrossOccurrences"):
            b.best()
        for other in (dense, hits, selfb):
            other.run()
            failed, err = _view_fails(engine, L.edlibAmdBatchCrossOccurrences, other._h, engine.CrossOccurrences())
            assert failed and "edlibAmdBatchCrossOccurrences" in err, err
        b.run()
        again = b.occurrences()
        assert np.array_equal(first["targetOffsets"], again["targetOffsets"])
        for f in M.FIELDS:
            assert np.array_equal(first[f], again[f]), f
        M.assert_equal(again, M.occurrences(qs, ts, 1))
        assert len(again["query"]) > 0
    finally:
        for x in (b, dense, hits, selfb):
            x.close()


def test_find_all_cross(engine):
    occ = engine.find_all_cross([b"ACGT"], [b"ACGTTTACGT", b"", b"CCCC"], 0)
    assert occ["targetOffsets"].tolist() == [0, 2, 2, 2]
    assert occ["firstEnd"].tolist() == [3, 9] and occ["query"].tolist() == [0, 0]
