"""GPU: the K nearest neighbours of every sequence of a self batch (edlibAmdBatchSelfNeighbors, SelfBatch.neighbors, knn).
The distances of self batches are held against the reference by test_gpu_self*.py; here the SELECTION is held three ways:
against neighbors_model() fed with the reference's condensed distances (ref_condensed of test_gpu_self.py, the checker),
against the model fed with the batch's own condensed() / hits() view, and against the nearest() view (columns 0 and 1).
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cross import _rand
from test_gpu_self import csr_of, mixed, ref_condensed
from test_gpu_self_strands import ref_both

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 63, 64)
FIELDS = ("count", "neighbor", "distance")


def model_of_condensed(engine, n, cond, K, level):
    i, j = np.triu_indices(n, 1)
    return engine.neighbors_model(n, np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([cond, cond]), K, level)


def model_of_hits(engine, n, h, K, level):
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    p, d = h["partner"], h["editDistance"]
    return engine.neighbors_model(n, np.concatenate([row, p]), np.concatenate([p, row]), np.concatenate([d, d]), K, level)


def assert_rows(got, want, ctx):
    for f in FIELDS:
        assert got[f].dtype == np.int32 and got[f].shape == want[f].shape, (f, ctx, got[f].shape, want[f].shape)
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (f, ctx, [(tuple(x), int(got[f][tuple(x)]), int(want[f][tuple(x)])) for x in bad[:5]])
    past = np.arange(got["neighbor"].shape[1])[None, :] >= got["count"][:, None]
    assert np.all(got["neighbor"][past] == -1) and np.all(got["distance"][past] == -1), ctx


def assert_identities(b, K):
    """max_distance = -1: columns 0 and 1 repeat the nearest view"""
    got, near = b.neighbors(K), b.nearest()
    assert np.array_equal(got["neighbor"][:, 0], near["nearest"])
    assert np.array_equal(got["distance"][:, 0], near["nearestDistance"])
    if K > 1:
        assert np.array_equal(got["distance"][:, 1], near["secondDistance"])


def check_batch(engine, b, n, ref, k, levels=(-1,), Ks=KS):
    """one Run: every K at every level against the reference and against the batch's own view, then the identities"""
    b.run()
    own = b.hits() if b.is_hits else b.condensed()
    for K in Ks:
        for level in levels:
            got = b.neighbors(K, level)
            assert "strand" not in got or b.both_strands
            # (level < 0: every pair the batch reports -- the reference's vector holds -1 for the others)
            assert_rows(got, model_of_condensed(engine, n, ref, K, level), ("ref", n, k, K, level))
            mine = model_of_hits(engine, n, own, K, level) if b.is_hits else model_of_condensed(engine, n, own, K, level)
            assert_rows(got, mine, ("own view", n, k, K, level))
        assert_identities(b, K)


def both_kinds(engine, seqs, ref_by_k, dense_k, hits_k, levels=lambda k: (-1,), Ks=KS, strands="forward"):
    for hits, k in [(False, k) for k in dense_k] + [(True, k) for k in hits_k]:
        b = engine.SelfBatch(seqs, k=k, hits=hits, strands=strands)
        try:
            check_batch(engine, b, len(seqs), ref_by_k[k], k, levels(k), Ks)
        finally:
            b.close()


# ---- 1. rows without a partner, with fewer than K, exactly K, K + 1, 63, 64, 65 and more

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 66, 129])
def test_row_lengths_around_k_and_the_chunk(engine, checker, n):
    rng = np.random.default_rng(100 + n)
    seqs = [_rand(rng, int(m), b"ACGT") for m in rng.integers(20, 41, size=n)]
    # k = -1 and k = 40 (no pair of these is further apart): every row has n - 1 partners; k = 14: sparse rows
    ref = {k: ref_condensed(seqs, k) for k in (-1, 14, 40)}
    assert np.all(ref[40] >= 0) and (n < 63 or (0 < np.count_nonzero(ref[14] >= 0) < len(ref[14])))
    both_kinds(engine, seqs, ref, dense_k=(-1, 14), hits_k=(14, 40), levels=lambda k: (-1,) if k < 0 else (-1, k // 2, k))


# ---- 2. the mixed set: three word groups, duplicates, empties; every level from one Run; the refusal above k

def test_mixed_set_every_level_from_one_run(engine, checker):
    seqs, ref = mixed()
    both_kinds(engine, seqs, ref, dense_k=(-1, 3), hits_k=(0, 3), levels=lambda k: (-1, 0, 1, k) if k > 0 else (-1, 0),
               Ks=(1, 5, 64))
    # a dense batch at k = -1 takes every level: level 3 of it is the k = 3 reference
    b = engine.SelfBatch(seqs, k=-1)
    try:
        b.run()
        for level in (0, 1, 3):
            want = np.where(ref[-1] <= level, ref[-1], -1)
            assert_rows(b.neighbors(5, level), model_of_condensed(engine, len(seqs), want, 5, -1), ("levels of k = -1", level))
    finally:
        b.close()


@pytest.mark.parametrize("hits", [False, True])
def test_max_distance_above_k_is_refused_and_changes_nothing(engine, hits):
    seqs, _ = mixed()
    b = engine.SelfBatch(seqs, k=3, hits=hits)
    try:
        with pytest.raises(RuntimeError, match="Run it first"):
            b.neighbors(3)
        st = b.run()
        near, nb = b.nearest(copy=False), b.neighbors(5, copy=False)
        keep = [near[f].copy() for f in near] + [nb[f].copy() for f in FIELDS]
        with pytest.raises(RuntimeError, match="maxDistance 4 is above the batch's k = 3"):
            b.neighbors(5, 4)
        for K in (0, 65):
            with pytest.raises(RuntimeError, match="K must be 1..64"):
                b.neighbors(K)
        # the views taken before, and the pointers held from them, are as they were; so are the statistics
        now = [near[f] for f in near] + [nb[f] for f in FIELDS]
        assert all(np.array_equal(a, c) for a, c in zip(keep, now))
        assert all(np.array_equal(b.nearest()[f], near[f]) for f in near)
        assert b.stats() == st
        out = engine.Neighbors()
        assert engine.lib().edlibAmdBatchCrossNeighbors(b._h, 3, -1, C.byref(out)) != 0
        assert "not a cross batch" in engine.last_error()
    finally:
        b.close()


# ---- 3. more than 64 candidates at distance 0: the index alone decides

def test_seventy_copies_order_by_index(engine, checker):
    rng = np.random.default_rng(31)
    one = _rand(rng, 30, b"ACGT")
    seqs = [one] * 70 + [_rand(rng, int(m), b"ACGT") for m in rng.integers(25, 36, size=30)]
    seqs = [seqs[int(o)] for o in rng.permutation(len(seqs))]
    ref = {k: ref_condensed(seqs, k) for k in (-1, 2)}
    both_kinds(engine, seqs, ref, dense_k=(-1,), hits_k=(2,))
    copies = np.array([i for i, s in enumerate(seqs) if s == one])
    b = engine.SelfBatch(seqs, k=2, hits=True)
    try:
        b.run()
        got = b.neighbors(64)
        for i in copies[:3]:
            assert got["count"][i] == 64 and np.all(got["distance"][i] == 0)
            assert np.array_equal(got["neighbor"][i], copies[copies != i][:64])
    finally:
        b.close()


# ---- 4. row 0's distances fall / rise with the index: every chunk replaces the list / nothing enters after the first

@pytest.mark.parametrize("rising", [False, True])
def test_monotone_rows(engine, checker, rising):
    rng = np.random.default_rng(41)
    base = bytearray(_rand(rng, 150, b"AC"))
    n = 141
    seqs = [bytes(base)]
    for j in range(1, n):
        s = bytearray(base)
        for p in range(j if rising else n - j):                       # substitutions no alignment of A / C can explain away
            s[p] = ord("G")
        seqs.append(bytes(s))
    ref = {k: ref_condensed(seqs, k) for k in (-1, 150)}
    d0 = ref[-1][:n - 1]
    assert np.all(np.diff(d0) > 0) if rising else np.all(np.diff(d0) < 0)
    both_kinds(engine, seqs, ref, dense_k=(-1,), hits_k=(150,), Ks=(1, 5, 64))


# ---- 5. a hit list without a hit: every row is empty

def test_hit_list_without_hits(engine, checker):
    rng = np.random.default_rng(51)
    seqs = [_rand(rng, 30, b"ACGT") for _ in range(70)]
    ref = ref_condensed(seqs, 0)
    assert np.all(ref == -1)
    b = engine.SelfBatch(seqs, k=0, hits=True)
    try:
        b.run()
        for K in (1, 64):
            got = b.neighbors(K)
            assert got["count"].tolist() == [0] * 70
            assert np.all(got["neighbor"] == -1) and np.all(got["distance"] == -1) and got["neighbor"].shape == (70, K)
    finally:
        b.close()


@pytest.mark.parametrize("seqs", [[], [b"ACGT"], [b""], [b"", b""]])
def test_sets_without_a_pair(engine, seqs):
    n = len(seqs)
    for hits, k in ((False, -1), (True, 1)):
        b = engine.SelfBatch(seqs, k=k, hits=hits)
        try:
            b.run()
            got = b.neighbors(2)
            assert got["count"].shape == (n,) and got["neighbor"].shape == (n, 2)
            assert got["count"].tolist() == ([1, 1] if n == 2 else [0] * n)
            if n == 2:
                assert got["neighbor"].tolist() == [[1, -1], [0, -1]] and got["distance"].tolist() == [[0, -1], [0, -1]]
        finally:
            b.close()


# ---- 6. pairs the kernel did not answer: 300-base sequences, an empty one, the 17-symbol set

def test_pairs_of_the_other_routes(engine, checker):
    rng = np.random.default_rng(17)                                   # (the set of test_gpu_self.test_self_other_routes)
    seqs = [_rand(rng, int(m), b"ACGT") for m in rng.integers(1, 200, size=37)]
    long_ = _rand(rng, 300, b"ACGT")
    seqs[5], seqs[20] = long_, long_[:150] + b"T" + long_[150:299]
    seqs += [_rand(rng, 300, b"ACGT"), b"", seqs[7]]
    ref = {k: ref_condensed(seqs, k) for k in (-1, 5)}
    both_kinds(engine, seqs, ref, dense_k=(-1, 5), hits_k=(5,), Ks=(1, 5, 64))
    for hits in (False, True):
        b = engine.SelfBatch(seqs, k=5, hits=hits)
        try:
            st = b.run()
            assert st["path"] & 2
            got = b.neighbors(3)
            # 5 and 20 are 300 bases long: only the internal pair batch answered their pair
            assert got["neighbor"][5, 0] == 20 and got["neighbor"][20, 0] == 5 and 0 < got["distance"][5, 0] <= 5
        finally:
            b.close()
    prot = b"ACDEFGHIKLMNPQRST"                                       # 17 symbols: every pair through the pair batch
    seqs = [_rand(rng, int(m), prot) for m in rng.integers(0, 80, size=10)] + [prot, prot[:-1]]
    ref = {k: ref_condensed(seqs, k) for k in (-1, 3)}
    both_kinds(engine, seqs, ref, dense_k=(-1, 3), hits_k=(3,), Ks=(1, 5, 64))


# ---- 7. both strands: the combined distances, and the strand byte of every reported pair

def test_both_strands(engine, checker):
    seqs, _ = mixed()
    seqs = [engine.reverse_complement(s) if i % 2 else s for i, s in enumerate(seqs)]
    n = len(seqs)
    rows = np.arange(n)[:, None]
    for hits, k in ((False, -1), (False, 3), (True, 3)):
        ed, strand = ref_both(engine, seqs, k)
        b = engine.SelfBatch(seqs, k=k, hits=hits, strands="both")
        try:
            check_batch(engine, b, n, ed, k, (-1,) if k < 0 else (-1, 1, k), Ks=(1, 5, 64))
            s = b.strands()
            if hits:
                # where pair (lo, hi) lies in the list
                h = b.hits()
                at = np.full((n, n), -1, dtype=np.int64)
                at[np.repeat(np.arange(n), np.diff(h["rowOffsets"])), h["partner"]] = np.arange(len(h["partner"]))
            for K in (1, 5, 64):
                got = b.neighbors(K)
                assert got["strand"].dtype == np.uint8 and got["strand"].shape == (n, K)
                have = got["neighbor"] >= 0
                nbr = np.maximum(got["neighbor"], 0)
                lo, hi = np.minimum(rows, nbr), np.maximum(rows, nbr)
                if hits:
                    assert np.all(at[lo, hi][have] >= 0)
                    mine = s["hitStrand"][np.maximum(at[lo, hi], 0)]
                else:
                    mine = s["pairStrand"][engine.condensed_index(n, lo, np.where(have, hi, lo + 1))]
                want = strand[engine.condensed_index(n, lo, np.where(have, hi, lo + 1))]
                assert np.array_equal(got["strand"][have], mine[have]), (hits, k, K)
                assert np.array_equal(got["strand"][have], want[have]), (hits, k, K)
                assert np.all(got["strand"][~have] == 0)
            assert (got["strand"][have] & 1).any() and not (got["strand"][have] & 1).all()
        finally:
            b.close()


# ---- 8. calls in a row, and after a second Run

@pytest.mark.parametrize("hits", [False, True])
def test_calls_in_a_row_and_after_another_run(engine, checker, hits):
    seqs, ref = mixed()
    n = len(seqs)
    b = engine.SelfBatch(seqs, k=3, hits=hits)
    try:
        st = b.run()
        a5, a64, a2 = b.neighbors(5), b.neighbors(64), b.neighbors(2, 1)
        assert_rows(a5, model_of_condensed(engine, n, ref[3], 5, -1), "first K = 5")
        assert_rows(a64, model_of_condensed(engine, n, ref[3], 64, -1), "then K = 64")
        assert_rows(a2, model_of_condensed(engine, n, ref[3], 2, 1), "then K = 2 at level 1")
        assert b.stats() == st                                        # a neighbours call leaves the statistics alone
        held = b.neighbors(5, copy=False)
        assert all(np.array_equal(held[f], a5[f]) for f in FIELDS)
        b.run()
        assert_rows(b.neighbors(64), a64, "after the second Run")
        assert_rows(b.neighbors(5), a5, "and K = 5 again")
        assert_identities(b, 5)
    finally:
        b.close()


def test_knn_one_shot(engine, checker):
    seqs, ref = mixed()
    n = len(seqs)
    assert_rows(engine.knn(seqs, 4), model_of_condensed(engine, n, ref[-1], 4, -1), "knn over all pairs")
    assert_rows(engine.knn(seqs, 4, k=3), model_of_condensed(engine, n, ref[3], 4, -1), "knn within 3")
    got = engine.knn(seqs, 2, k=3, strands="both")
    assert set(got) == {"count", "neighbor", "distance", "strand"}
    assert_rows(got, model_of_condensed(engine, n, ref_both(engine, seqs, 3)[0], 2, -1), "knn on both strands")
    assert csr_of(n, ref[3])["rowOffsets"][-1] > 0                    # (the set has pairs within 3 at all)
