"""GPU: the K nearest queries of every target of a cross batch (edlibAmdBatchCrossNeighbors, CrossBatch.neighbors).  The
cells of cross batches are held against the reference by test_gpu_cross*.py; here the SELECTION is held three ways: against
neighbors_model() fed with the checker's cells (ref_cells / check_cells of test_gpu_cross.py, ref_both of
test_gpu_cross_strands.py), against the model fed with the batch's own matrix() / hits() view, and against the best() view
(columns 0 and 1).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cross import _rand, check_cells, ref_cells
from test_gpu_cross_strands import _mutate, ref_both

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 63, 64)
FIELDS = ("count", "neighbor", "distance")


def model_of_matrix(engine, ed, K, level):
    nt, nq = ed.shape
    t, q = np.divmod(np.arange(nt * nq), max(nq, 1))
    return engine.neighbors_model(nt, t, q, ed.reshape(-1), K, level)


def model_of_hits(engine, nt, h, K, level):
    row = np.repeat(np.arange(nt), np.diff(h["targetOffsets"]))
    return engine.neighbors_model(nt, row, h["query"], h["editDistance"], K, level)


def assert_rows(got, want, ctx):
    for f in FIELDS:
        assert got[f].dtype == np.int32 and got[f].shape == want[f].shape, (f, ctx, got[f].shape, want[f].shape)
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (f, ctx, [(tuple(x), int(got[f][tuple(x)]), int(want[f][tuple(x)])) for x in bad[:5]])


def assert_identities(b, K):
    got, best = b.neighbors(K), b.best()
    assert np.array_equal(got["neighbor"][:, 0], best["bestQuery"])
    assert np.array_equal(got["distance"][:, 0], best["bestQueryDistance"])
    if K > 1:
        assert np.array_equal(got["distance"][:, 1], best["secondQueryDistance"])


def barcodes_and_reads(rng, nq, nt, mode):
    """nq barcodes of 24 bases; nt targets that carry one of them with 0 .. 2 substitutions -- inside 60 random bases for
    HW, alone for NW --, target 1 without any (poly-T), a few targets that carry a barcode's reverse complement"""
    import edlib_amd
    queries = [_rand(rng, 24, b"ACGT") for _ in range(nq)]
    targets = []
    for t in range(nt):
        bc = _mutate(rng, queries[int(rng.integers(0, nq))], t % 3)
        if t % 7 == 3:
            bc = edlib_amd.reverse_complement(bc)
        targets.append(bc if mode == "NW" else _rand(rng, 20, b"ACGT") + bc + _rand(rng, 16, b"ACGT"))
    targets[1] = b"T" * len(targets[1])
    return queries, targets


def check_kind(engine, queries, targets, mode, k, hits, both, ed, strand):
    """one batch of one kind against the reference's matrix `ed` (and strand bytes), its own view and its best view"""
    nt = len(targets)
    b = engine.CrossBatch(queries, targets, mode=mode, k=k, hits=hits, strands="both" if both else "forward")
    try:
        b.run()
        if not hits and not both:
            check_cells(b, queries, targets, mode, k)                 # (the checker's own call: the matrix is the reference's)
        own = b.hits() if hits else b.matrix()["editDistance"]
        s = b.strands() if both else None
        if hits:
            at = np.full((nt, max(len(queries), 1)), -1, dtype=np.int64)
            at[np.repeat(np.arange(nt), np.diff(own["targetOffsets"])), own["query"]] = np.arange(len(own["query"]))
        for K in KS:
            for level in ((-1,) if k < 0 else (-1, 0, 1, k)):
                ctx = (mode, k, hits, both, K, level)
                got = b.neighbors(K, level)
                assert ("strand" in got) == both
                assert_rows(got, model_of_matrix(engine, ed, K, level), ("ref",) + ctx)
                mine = model_of_hits(engine, nt, own, K, level) if hits else model_of_matrix(engine, own, K, level)
                assert_rows(got, mine, ("own view",) + ctx)
                if both:
                    have = got["neighbor"] >= 0
                    rows, nbr = np.arange(nt)[:, None], np.maximum(got["neighbor"], 0)
                    want = np.broadcast_to(strand[rows, nbr], have.shape)
                    assert got["strand"].dtype == np.uint8 and got["strand"].shape == have.shape
                    assert np.array_equal(got["strand"][have], want[have]), ctx
                    mine = s["hitStrand"][np.maximum(at[rows, nbr], 0)] if hits else s["cellStrand"][rows, nbr]
                    assert np.array_equal(got["strand"][have], mine[have]), ctx
                    assert np.all(got["strand"][~have] == 0)
            assert_identities(b, K)
    finally:
        b.close()


@pytest.mark.parametrize("nq", [1, 5, 64, 65, 96])
@pytest.mark.parametrize("nt", [9, 130])
def test_shapes_modes_and_kinds(engine, checker, nt, nq):
    for mode, k in (("HW", 3), ("HW", -1), ("NW", 2)):
        rng = np.random.default_rng(nt * 1000 + nq * 10 + k + 1)
        queries, targets = barcodes_and_reads(rng, nq, nt, mode)
        fwd, _, cells, strand = ref_both(queries, targets, mode, k)
        if k >= 0:
            assert np.all(cells["editDistance"][1] == -1)                 # the target with no hit
            assert (cells["editDistance"] >= 0).any() and (strand & 1).any()
        for both in (False, True):
            ed = (cells if both else fwd)["editDistance"]
            check_kind(engine, queries, targets, mode, k, False, both, ed, strand)
            if k >= 0:
                check_kind(engine, queries, targets, mode, k, True, both, ed, strand)


def test_no_queries_and_no_targets(engine):
    rng = np.random.default_rng(2)
    seqs = [_rand(rng, 24, b"ACGT") for _ in range(7)]
    for hits, k in ((False, -1), (True, 3)):
        for both in ("forward", "both"):
            b = engine.CrossBatch([], seqs, mode="HW", k=k, hits=hits, strands=both)
            try:
                b.run()
                got = b.neighbors(3)
                assert got["count"].tolist() == [0] * 7 and got["neighbor"].shape == (7, 3) and np.all(got["neighbor"] == -1)
                assert np.all(got["distance"] == -1)
            finally:
                b.close()
            b = engine.CrossBatch(seqs, [], mode="HW", k=k, hits=hits, strands=both)
            try:
                b.run()
                got = b.neighbors(3)
                assert got["count"].shape == (0,) and got["neighbor"].shape == (0, 3) and got["distance"].shape == (0, 3)
            finally:
                b.close()


@pytest.mark.parametrize("hits", [False, True])
def test_streamed_targets_need_their_run(engine, checker, hits):
    rng = np.random.default_rng(5)
    queries, first = barcodes_and_reads(rng, 20, 12, "HW")
    second = [_mutate(rng, queries[t % 20], t % 3) + _rand(rng, 30, b"ACGT") for t in range(30)]
    b = engine.CrossBatch(queries, first, mode="HW", k=3, hits=hits)
    try:
        with pytest.raises(RuntimeError, match="Run it first"):
            b.neighbors(3)
        b.run()
        tq = [(t, q) for t in range(12) for q in range(20)]
        ed = np.asarray(ref_cells(queries, first, "HW", 3, None, tq)[0]).reshape(12, 20)
        assert_rows(b.neighbors(5), model_of_matrix(engine, ed, 5, -1), "first set")
        b.set_targets(second)
        with pytest.raises(RuntimeError, match="Run it first"):
            b.neighbors(5)                                            # new targets since the last Run: not run
        b.run()
        tq = [(t, q) for t in range(30) for q in range(20)]
        ed = np.asarray(ref_cells(queries, second, "HW", 3, None, tq)[0]).reshape(30, 20)
        for K in (1, 5, 64):
            assert_rows(b.neighbors(K), model_of_matrix(engine, ed, K, -1), ("second set", K))
        assert_identities(b, 5)
    finally:
        b.close()


def test_refusals_leave_the_batch_as_it_was(engine):
    rng = np.random.default_rng(6)
    queries, targets = barcodes_and_reads(rng, 20, 12, "HW")
    occ = engine.CrossBatch(queries, targets, mode="HW", k=3, occurrences=True)
    try:
        occ.run()
        with pytest.raises(RuntimeError, match="occurrence batch"):
            occ.neighbors(3)
        assert occ.occurrences()["targetOffsets"].shape == (13,)
    finally:
        occ.close()
    b = engine.CrossBatch(queries, targets, mode="HW", k=3)
    try:
        st = b.run()
        best, nb = b.best(copy=False), b.neighbors(5, copy=False)
        keep = [best[f].copy() for f in best] + [nb[f].copy() for f in FIELDS]
        with pytest.raises(RuntimeError, match="maxDistance 4 is above the batch's k = 3"):
            b.neighbors(5, 4)
        for K in (0, 65):
            with pytest.raises(RuntimeError, match="K must be 1..64"):
                b.neighbors(K)
        out = engine.Neighbors()
        assert engine.lib().edlibAmdBatchSelfNeighbors(b._h, 3, -1, C.byref(out)) != 0
        assert "not a self batch" in engine.last_error()
        assert all(np.array_equal(a, c) for a, c in zip(keep, [best[f] for f in best] + [nb[f] for f in FIELDS]))
        assert b.stats() == st
    finally:
        b.close()
