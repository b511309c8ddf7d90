"""CPU: the model of occurrence cross batches (cross_occ_model.occurrences) on cases worked by hand, on the edge cases of
the definition, against the textbook bottom row (hits_model.d_row), and tied to the oracle cell by cell: with
r = edlibAlign(q, t, HW, k), r is -1 exactly where the cell has no occurrence, otherwise the least occurrence distance is
r's, every non-negative end location of r lies in an occurrence of that distance, and those occurrences' numLocations sum
to the number of such locations.  (The tie runs over non-empty queries and targets: the reference answers an empty query
with the single end location -1, and the definition gives the empty cases their own rule.)"""
import numpy as np
import pytest

import cross_occ_model as M
import hits_model as H


def _rand(rng, n, chars=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(chars, dtype=np.uint8), size=n).tolist())


def test_by_hand():
    # ACGT ends exactly at the columns 3 and 9; at k = 1 the neighbouring columns join each run
    occ = M.occurrences([b"ACGT"], [b"ACGTTTACGT"], 0)
    assert occ["targetOffsets"].tolist() == [0, 2]
    assert M.cell_runs(occ, 0, 0) == [(3, 3, 0, 3, 1), (9, 9, 0, 9, 1)]
    occ = M.occurrences([b"ACGT"], [b"ACGTTTACGT"], 1)
    assert M.cell_runs(occ, 0, 0) == [(2, 4, 0, 3, 1), (8, 9, 0, 9, 1)]
    # two queries, two targets: (target, query, firstEnd) order, target-relative columns
    occ = M.occurrences([b"GG", b"AC"], [b"ACAC", b"TGGT"], 0)
    assert occ["targetOffsets"].tolist() == [0, 2, 3]
    assert occ["query"].tolist() == [1, 1, 0]
    assert occ["firstEnd"].tolist() == [1, 3, 2]
    M.assert_ordered(occ, 2)


def test_edge_cases():
    qs, ts = [b"", b"ACG", b"T"], [b"", b"ACGACG", b"A"]
    occ = M.occurrences(qs, ts, 0)
    assert occ["targetOffsets"][1] == 0                                   # an empty target holds no occurrence
    assert M.cell_runs(occ, 1, 0) == [(0, 5, 0, 0, 6)]                    # the empty query: once, over the whole target
    assert M.cell_runs(occ, 2, 0) == [(0, 0, 0, 0, 1)]
    assert M.cell_runs(occ, 1, 1) == [(2, 2, 0, 2, 1), (5, 5, 0, 5, 1)]
    assert M.cell_runs(occ, 1, 2) == [] and M.cell_runs(occ, 2, 2) == []
    # k >= m: one run over every non-empty target
    occ = M.occurrences(qs, ts, 3)
    for t, n in ((1, 6), (2, 1)):
        for q in range(3):
            runs = M.cell_runs(occ, t, q)
            assert len(runs) == 1 and runs[0][:2] == (0, n - 1), (t, q, runs)
    assert M.cell_runs(occ, 1, 1)[0][2:] == (0, 2, 2)
    assert occ["targetOffsets"].tolist() == [0, 0, 3, 6]
    for nq, nt in ((0, 2), (2, 0), (0, 0)):
        occ = M.occurrences(qs[:nq], ts[:nt], 1)
        assert len(occ["query"]) == 0 and occ["targetOffsets"].tolist() == [0] * (nt + 1)


def test_against_textbook_rows():
    rng = np.random.default_rng(3)
    eq = [("N", c) for c in "ACGT"]
    queries = [_rand(rng, int(n), b"ACGTN") for n in (1, 5, 33, 64, 65, 70)]
    targets = [_rand(rng, int(n), b"ACGTN") for n in (0, 1, 9, 40, 130)]
    for k, e in ((0, None), (2, None), (3, eq)):
        occ = M.occurrences(queries, targets, k, e)
        M.assert_ordered(occ, len(queries))
        for t, tg in enumerate(targets):
            for q, qu in enumerate(queries):
                assert M.cell_runs(occ, t, q) == H.hits(H.d_row(qu, tg, e), k), (k, t, q)


@pytest.mark.parametrize("k", [0, 2, 5])
def test_tied_to_the_oracle(oracle, k):
    rng = np.random.default_rng(40 + k)
    eq = [("N", c) for c in "ACGT"] if k == 2 else None
    chars = b"ACGTN" if eq else b"ACGT"
    targets = []
    queries = [_rand(rng, int(n), chars) for n in (3, 8, 20, 33, 64, 90)]
    for i in range(6):
        body = bytearray(_rand(rng, int(rng.integers(30, 200)), chars))
        for q in (queries[i], queries[(i + 2) % 6]):                      # planted copies, one of them mutated
            at = int(rng.integers(0, len(body)))
            body[at:at] = q
        if len(body) > 10:
            body[5] = body[6]
        targets.append(bytes(body))
    targets.append(queries[1] + queries[1])                               # two copies back to back
    occ = M.occurrences(queries, targets, k, eq)
    cells = 0
    for t, tg in enumerate(targets):
        for q, qu in enumerate(queries):
            r = oracle.align(qu, tg, "HW", "distance", k, eq_pairs=eq)
            runs = M.cell_runs(occ, t, q)
            assert (r["editDistance"] == -1) == (len(runs) == 0), (t, q, r, runs)
            cells += 1
            if not runs:
                continue
            assert min(x[2] for x in runs) == r["editDistance"], (t, q)
            best = [x for x in runs if x[2] == r["editDistance"]]
            ends = [e for e in r["endLocations"] if e >= 0]
            for e in ends:
                assert any(f <= e <= l for f, l, _, _, _ in best), (t, q, e, best)
            assert sum(x[4] for x in best) == len(ends), (t, q, best, ends)
    assert cells == 42
