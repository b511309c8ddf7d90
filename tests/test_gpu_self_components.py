"""GPU: the connected components of self batches (edlibAmdBatchSelfComponents, SelfBatch.components(), cluster_within()),
labelled on the device from the finished hit list or the condensed vector.  The distances every case rests on are the
checker's (the compiled reference where it travelled), the expected components are self_components_model() over them,
and what a case assumes of its set -- families apart, a chain whose non-adjacent members are above k -- is asserted on the
checker's numbers first."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cross import _rand
from test_gpu_self import csr_of, ref_condensed
from test_gpu_self_strands import ref_both

pytestmark = pytest.mark.gpu

ARRAYS = ("label", "componentSize", "componentOffsets", "members")
ACGT = b"ACGT"


def model(engine, n, cond, level):
    """the components of a condensed vector of distances at a level"""
    c = csr_of(n, cond)
    return engine.self_components_model(n, c["rowOffsets"], c["partner"], c["editDistance"], level)


def assert_same(got, want, what=""):
    assert got["numComponents"] == want["numComponents"], (what, got["numComponents"], want["numComponents"])
    for f in ARRAYS:
        assert got[f].dtype == np.int32 and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def components(engine, seqs, k, hits, levels=(-1,), strands="forward", eqs=None):
    """[components(level, members=True) for level in levels] of one Run, and its stats"""
    b = engine.SelfBatch(seqs, k=k, hits=hits, strands=strands, additionalEqualities=eqs)
    try:
        st = b.run()
        return [b.components(level, members=True) for level in levels], st
    finally:
        b.close()


def substitute(rng, s, positions):
    """s with another base at each of the positions"""
    s = bytearray(s)
    for p in positions:
        s[p] = ACGT[(ACGT.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def families(rng):
    """6 families x 5 sequences of 20 bases -- a centre and four copies with one substitution -- in shuffled order; the
    family of every sequence"""
    seqs, fam = [], []
    for f in range(6):
        centre = _rand(rng, 20, ACGT)
        seqs += [centre] + [substitute(rng, centre, [int(rng.integers(0, 20))]) for _ in range(4)]
        fam += [f] * 5
    order = rng.permutation(len(seqs))
    return [seqs[int(o)] for o in order], np.array(fam)[order]


def assert_families(fam, cond, inside, between):
    """the precondition: pairs of one family are within `inside`, pairs of two families at `between` or more"""
    i, j = np.triu_indices(len(fam), 1)
    same = fam[i] == fam[j]
    assert np.all((cond[same] >= 0) & (cond[same] <= inside)) and np.all(cond[~same] >= between)


def family_labels(fam):
    return np.array([int(np.flatnonzero(fam == f)[0]) for f in fam], dtype=np.int32)


def test_components_families(engine, checker):
    seqs, fam = families(np.random.default_rng(1))
    n = len(seqs)
    assert n == 30
    assert_families(fam, ref_condensed(seqs, -1), 2, 6)
    want = model(engine, n, ref_condensed(seqs, 2), 2)
    assert want["numComponents"] == 6 and np.array_equal(want["label"], family_labels(fam))
    (h,), _ = components(engine, seqs, 2, True)
    (d,), _ = components(engine, seqs, 2, False)
    assert_same(h, want, "hits")
    assert_same(d, want, "dense")
    assert h["numComponents"] == d["numComponents"] == 6 and np.all(h["componentSize"] == 5)
    assert np.array_equal(engine.cluster_within(seqs, 2), want["label"])
    b = engine.SelfBatch(seqs, k=2, hits=True)                      # labels only: no members, the same labels
    try:
        b.run()
        c = b.components()
        assert sorted(c) == ["componentSize", "label", "numComponents"]
        assert np.array_equal(c["label"], want["label"]) and np.array_equal(c["componentSize"], want["componentSize"])
    finally:
        b.close()


def test_components_long_chain(engine, checker):
    """one component of diameter 199: long find paths, roots hooked again and again"""
    rng = np.random.default_rng(2)
    chain = [_rand(rng, 200, ACGT)]
    for t in range(199):
        chain.append(substitute(rng, chain[-1], [t]))
    order = rng.permutation(200)
    seqs = [chain[int(o)] for o in order]
    place = np.empty(200, dtype=np.int64)                           # index -> position in the chain
    place[np.arange(200)] = order
    ref = ref_condensed(seqs, 1)
    i, j = np.triu_indices(200, 1)
    adjacent = np.abs(place[i] - place[j]) == 1
    assert np.all(ref[adjacent] == 1) and np.all(ref[~adjacent] == -1)      # the precondition: a path, nothing else
    want = model(engine, 200, ref, 1)
    assert want["numComponents"] == 1 and not want["label"].any()
    alone = model(engine, 200, ref, 0)
    assert alone["numComponents"] == 200
    for hits in (True, False):
        (c1, c0), _ = components(engine, seqs, 1, hits, levels=(1, 0))
        assert_same(c1, want, hits)
        assert_same(c0, alone, hits)
        assert c1["componentSize"].tolist() == [200] * 200 and c0["label"].tolist() == list(range(200))


def test_components_levels_from_one_run(engine, checker):
    rng = np.random.default_rng(3)
    seqs = []
    for _ in range(8):                                               # a centre, a duplicate, and a path of 1, 2, 3 steps
        c = _rand(rng, 24, ACGT)
        p = [int(x) for x in rng.permutation(24)[:9]]
        seqs += [c, c, substitute(rng, c, p[:1]), substitute(rng, c, p[1:3]), substitute(rng, c, p[3:6])]
        seqs += [substitute(rng, seqs[-1], p[6:7]), substitute(rng, seqs[-2], p[7:9]), substitute(rng, seqs[-3], p[6:9])]
    seqs = [seqs[int(o)] for o in rng.permutation(len(seqs))]
    n = len(seqs)
    assert n == 64
    ref = ref_condensed(seqs, 3)
    assert all(np.count_nonzero(ref == d) >= 8 for d in (0, 1, 2, 3))        # duplicates, neighbours at 1, 2 and 3
    levels = (0, 1, 2, 3, -1)
    wants = [model(engine, n, ref, 3 if level < 0 else level) for level in levels]
    assert wants[0]["numComponents"] > wants[1]["numComponents"] > wants[3]["numComponents"]
    for hits in (True, False):
        b = engine.SelfBatch(seqs, k=3, hits=hits)
        try:
            b.run()
            got = [b.components(level, members=True) for level in levels]
            for level, g, w in zip(levels, got, wants):
                assert_same(g, w, (hits, level))
            assert_same(got[4], got[3], "level -1 is the batch's k")
            nc = [g["numComponents"] for g in got[:4]]
            assert nc == sorted(nc, reverse=True)
            # a level above k is refused, and what the last call returned still reads the same
            view = b.components(2, members=True, copy=False)
            kept = {f: view[f].copy() for f in ARRAYS}
            with pytest.raises(RuntimeError, match="maxDistance 4 is above the batch's k = 3"):
                b.components(4)
            for f in ARRAYS:
                assert np.array_equal(view[f], kept[f]) and np.array_equal(kept[f], wants[2][f]), f
            assert_same(b.components(0, members=True), wants[0], "after the refusal")
        finally:
            b.close()


def test_components_contention(engine):
    """2,096,128 edges into one tree of 2,048 vertices; the list grows in the first Run"""
    seq = b"ACGTTGCAACGTACGTTGCA"
    n = 2048
    b = engine.SelfBatch([seq] * n, k=0, hits=True)
    try:
        b.run()
        got = [b.components(members=True), b.components(0, members=True)]
        assert len(b.hits(copy=False)["partner"]) == 2_096_128
        b.run()
        got.append(b.components(members=True))
    finally:
        b.close()
    for c in got:
        assert c["numComponents"] == 1 and not c["label"].any() and np.all(c["componentSize"] == n)
        assert c["componentOffsets"].tolist() == [0, n] and np.array_equal(c["members"], np.arange(n))


def test_components_both_strands(engine, checker):
    seqs, fam = families(np.random.default_rng(5))
    seqs = [engine.reverse_complement(s) if x % 2 else s for x, s in enumerate(seqs)]
    n = len(seqs)
    i, j = np.triu_indices(n, 1)
    fwd = ref_condensed(seqs, 2)
    # the precondition of the one-strand split: inside a family, sequences of different orientation are above 2
    assert np.all(fwd[(fam[i] == fam[j]) & (i % 2 != j % 2)] == -1)
    split = model(engine, n, fwd, 2)
    assert split["numComponents"] > 6
    assert_families(fam, ref_both(engine, seqs, -1)[0], 2, 6)
    want = model(engine, n, ref_both(engine, seqs, 2)[0], 2)
    assert want["numComponents"] == 6 and np.array_equal(want["label"], family_labels(fam))
    for hits in (True, False):
        (one,), _ = components(engine, seqs, 2, hits)
        assert_same(one, split, ("forward", hits))
        (both,), _ = components(engine, seqs, 2, hits, strands="both")
        assert_same(both, want, ("both", hits))
    assert np.array_equal(engine.cluster_within(seqs, 2, strands="both"), want["label"])


def test_components_pairs_off_the_kernel(engine, checker):
    """the edges the internal pair batch answered are in the graph: sequences above 256 bases, a set of 17 symbols"""
    rng = np.random.default_rng(17)
    seqs = [_rand(rng, int(m), ACGT) for m in rng.integers(1, 200, size=37)]
    long_ = _rand(rng, 300, ACGT)
    seqs[5], seqs[20] = long_, long_[:150] + b"T" + long_[150:299]
    seqs += [long_[:299] + b"A", b"", seqs[7]]
    assert len(seqs) == 40 and sum(1 for s in seqs if len(s) == 300) == 3
    ref = ref_condensed(seqs, 5)
    want = model(engine, 40, ref, 5)
    assert want["label"][20] == 5 and want["label"][37] == 5 and want["label"][39] == 7     # joined by the pair batch's edges
    for hits in (True, False):
        (c,), st = components(engine, seqs, 5, hits)
        assert st["path"] & 8 and st["path"] & 2
        assert_same(c, want, hits)
    prot = b"ACDEFGHIKLMNPQRST"                                       # 17 symbols: every pair through the pair batch
    seqs = [_rand(rng, int(m), prot) for m in rng.integers(0, 80, size=10)] + [prot, prot[:-1], prot[1:]]
    ref = ref_condensed(seqs, 3)
    want = model(engine, len(seqs), ref, 3)
    assert want["label"][11] == 10 and want["label"][12] == 10
    for hits in (True, False):
        (c,), st = components(engine, seqs, 3, hits)
        assert not (st["path"] & 8) and st["path"] & 2
        assert_same(c, want, hits)


def test_components_empty_sequences_and_tiny_sets(engine, checker):
    for hits, k in ((True, 1), (False, -1), (False, 1)):
        (c,), _ = components(engine, [], k, hits)
        assert c["numComponents"] == 0 and c["componentOffsets"].tolist() == [0]
        assert all(c[f].shape == (0,) for f in ("label", "componentSize", "members"))
        (c,), _ = components(engine, [b"ACGT"], k, hits)
        assert c["numComponents"] == 1 and c["componentOffsets"].tolist() == [0, 1]
        assert c["label"].tolist() == [0] and c["componentSize"].tolist() == [1] and c["members"].tolist() == [0]
        # two empty sequences: distance 0, one component at any level
        levels = (-1, 0) if k < 0 else (-1, 0, 1)
        got, _ = components(engine, [b"", b""], k, hits, levels=levels)
        for c in got:
            assert c["numComponents"] == 1 and c["label"].tolist() == [0, 0] and c["componentSize"].tolist() == [2, 2]
    # an empty sequence is reported at the other's length whatever k: under d <= level it joins lengths 1 and 2 only
    seqs = [_rand(np.random.default_rng(7), 30, ACGT), b"", b"A", b"AC"]
    b = engine.SelfBatch(seqs, k=2, hits=True)
    try:
        b.run()
        h = b.hits()
        assert h["partner"][:h["rowOffsets"][1]].tolist() == [1] and h["editDistance"][0] == 30      # reported, above k
        c = b.components(members=True)
        assert_same(c, engine.self_components_model(4, h["rowOffsets"], h["partner"], h["editDistance"], 2), "hits")
    finally:
        b.close()
    assert c["label"].tolist() == [0, 1, 1, 1] and c["numComponents"] == 2
    assert c["componentOffsets"].tolist() == [0, 1, 4] and c["members"].tolist() == [0, 1, 2, 3]
    (d,), _ = components(engine, seqs, 2, False)
    assert_same(d, c, "dense")
    (l0, l1), _ = components(engine, seqs, 2, True, levels=(0, 1))
    assert l0["label"].tolist() == [0, 1, 2, 3] and l1["label"].tolist() == [0, 1, 1, 1]
    # a dense batch at k = -1: every pair is reported, so level -1 is one component; level 2 is the model's
    rng = np.random.default_rng(8)
    seqs = [_rand(rng, 12, ACGT) for _ in range(6)]
    seqs += [substitute(rng, s, [3]) for s in seqs[:4]] + [b""]
    ref = ref_condensed(seqs, -1)
    (every, two), _ = components(engine, seqs, -1, False, levels=(-1, 2))
    assert every["numComponents"] == 1 and not every["label"].any()
    want = model(engine, len(seqs), ref, 2)
    assert 1 < want["numComponents"] < len(seqs)
    assert_same(two, want, "k = -1, level 2")


def test_components_state_and_refusals(engine):
    L = engine.lib()
    seqs = [b"ACGT", b"ACGA", b"TTTT", b"TTTT"]                      # 0 -1- 1, 2 -0- 3, the two pairs 3 and 4 apart
    d = engine.SelfBatch(seqs, k=2)
    h = engine.SelfBatch(seqs, k=2, hits=True)
    others = [engine.CrossBatch([b"ACGT"], [b"ACGA"], "NW"), engine.SharedBatch([b"ACGT"], b"TTACGTTT"),
              engine.PairBatch([b"ACGT"], [b"ACGA"]), engine.WindowBatch([b"ACGT"], b"TTACGTTT", [0], [0], [8])]
    try:
        out = engine.SelfComponents()
        for b in (d, h):                                             # before the first Run
            assert L.edlibAmdBatchSelfComponents(b._h, -1, 1, C.byref(out)) != 0
            assert "Run it first" in engine.last_error()
            with pytest.raises(RuntimeError, match="Run it first"):
                b.components()
        for b in others:
            b.run()
            assert L.edlibAmdBatchSelfComponents(b._h, -1, 1, C.byref(out)) != 0
            assert "self batch" in engine.last_error(), engine.last_error()
        d.run()
        h.run()
        for b in (d, h):
            assert L.edlibAmdBatchSelfComponents(b._h, -1, 3, None) != 0
            assert "null" in engine.last_error()
            assert L.edlibAmdBatchSelfComponents(b._h, -1, 4, C.byref(out)) != 0
            assert "unknown parts 4" in engine.last_error()
            assert L.edlibAmdBatchSelfComponents(b._h, 3, 1, C.byref(out)) != 0
            assert "above the batch's k = 2" in engine.last_error()
        # the other views' pinned memory is not touched by a components call
        views = {"hits": h.hits(copy=False), "near": h.nearest(copy=False), "cond": {"c": d.condensed(copy=False)},
                 "dnear": d.nearest(copy=False)}
        kept = {v: {f: np.array(a, copy=True) for f, a in views[v].items()} for v in views}
        st = (d.stats(), h.stats())
        for b in (d, h):
            c = b.components(members=True)
            assert c["label"].tolist() == [0, 0, 2, 2] and c["numComponents"] == 2
            assert L.edlibAmdBatchSelfComponents(b._h, -1, 2, C.byref(out)) == 0          # members alone: labels filled too
            assert out.numSequences == 4 and out.numComponents == 2 and out.label and out.componentSize
            assert out.componentOffsets and out.members
            assert L.edlibAmdBatchSelfComponents(b._h, -1, 1, C.byref(out)) == 0
            assert out.label and not out.componentOffsets and not out.members
        again = {"hits": h.hits(copy=False), "near": h.nearest(copy=False), "cond": {"c": d.condensed(copy=False)},
                 "dnear": d.nearest(copy=False)}
        for v in views:
            for f in views[v]:
                assert np.array_equal(views[v][f], kept[v][f]), (v, f)
                if isinstance(views[v][f], np.ndarray) and views[v][f].size:
                    assert again[v][f].ctypes.data == views[v][f].ctypes.data, (v, f)
        assert (d.stats(), h.stats()) == st
    finally:
        for b in [d, h] + others:
            b.close()
