"""GPU: grouped self batches (edlibAmdBatchCreateSelfHitsGrouped, SelfBatch(hits=True, groups=...)): only the pairs inside
a group exist, and every view reports what a hit-list self batch over each group alone would, in the indices of the whole
set.  Distances are compared with the checker (the compiled reference where it travelled) on the same-group pairs, the
index mapping with per-group SelfBatch runs through grouped_hits_model(), nearest / components / neighbours with the
numpy models fed with the reference's distances, the counters with the formulas of self_groups_cases.py."""
import numpy as np
import pytest

import self_groups_cases as SG
from test_gpu_self import NEAR, assert_csr, ref_pairs, run_hits

pytestmark = pytest.mark.gpu


def run_grouped(engine, seqs, groups, k, eqs=None):
    b = engine.SelfBatch(seqs, k=k, additionalEqualities=eqs, hits=True, groups=groups)
    try:
        st = b.run()
        return b.hits(), b.nearest(), st
    finally:
        b.close()


def ref_grouped(seqs, groups, k, eqs=None):
    """(first, second, ed): every same-group pair and the reference's distance at k"""
    first, second = SG.same_group_pairs(groups)
    return first, second, ref_pairs(seqs, first, second, k, eqs)


def assert_grouped(engine, seqs, groups, k, eqs=None, word_steps=True):
    n = len(seqs)
    first, second, ed = ref_grouped(seqs, groups, k, eqs)
    h, near, st = run_grouped(engine, seqs, groups, k, eqs)
    assert_csr(h, n, SG.csr_of_pairs(n, first, second, ed))
    want = engine.self_nearest_model(n, first, second, ed)
    for f in NEAR:
        assert np.array_equal(near[f], want[f]), f
    lens = [len(s) for s in seqs]
    assert st["cells"] == SG.grouped_cells(lens, groups)
    if word_steps:
        assert st["word_steps"] == SG.grouped_word_steps(lens, groups, k)
    return h, st, (first, second, ed)


_PLANTED = {}


def planted():
    if not _PLANTED:
        seqs, groups, marks = SG.planted_set()
        _PLANTED.update(seqs=seqs, groups=groups, marks=marks)
    return _PLANTED


@pytest.mark.parametrize("k", [0, 2, 5])
def test_planted_set(engine, checker, k):
    p = planted()
    seqs, groups, marks = p["seqs"], p["groups"], p["marks"]
    n = len(seqs)
    h, st, (first, second, ed) = assert_grouped(engine, seqs, groups, k)
    assert st["path"] == 8 and 0 < len(h["partner"]) < len(first)
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    listed = set(zip(row.tolist(), h["partner"].tolist()))
    # identical sequences in different groups are no hits; inside one group they are hits at distance 0
    for a in marks["across"]:
        for b in marks["across"]:
            assert (a, b) not in listed
            assert checker.align(seqs[a], seqs[b], "NW", "distance", k)["editDistance"] == 0
    for x, a in enumerate(marks["inside"]):
        for b in marks["inside"][x + 1:]:
            at = np.flatnonzero((row == a) & (h["partner"] == b))
            assert len(at) == 1 and h["editDistance"][at[0]] == 0
    assert np.all(groups[row] == groups[h["partner"]])
    # a SelfBatch(hits=True) per group, mapped back by the model
    per = {}
    for lab, part in SG.members_of(groups).items():
        per[lab] = run_hits(engine, [seqs[int(i)] for i in part], k)[0]
    want = engine.grouped_hits_model(groups, per)
    for f in want:
        assert np.array_equal(h[f], want[f]), f


def test_one_label_equals_the_ungrouped_batch(engine):
    p = planted()
    seqs = p["seqs"] + [b"", b"ACGT" * 70, b"ACGT" * 70 + b"A"]            # every route: empty, above 256 bases
    for k in (0, 3):
        h, near, st = run_grouped(engine, seqs, np.full(len(seqs), -9), k)
        h0, near0, st0 = run_hits(engine, seqs, k)
        for f in h0:
            assert np.array_equal(h[f], h0[f]), f
        for f in NEAR:
            assert np.array_equal(near[f], near0[f]), f
        for f in ("cells", "word_steps", "path", "scan_launches"):
            assert st[f] == st0[f], f
    b = engine.SelfBatch(seqs, k=3, hits=True, groups=np.zeros(len(seqs), dtype=np.int64))
    b0 = engine.SelfBatch(seqs, k=3, hits=True)
    try:
        b.run()
        b0.run()
        for level in (1, 3):
            c, c0 = b.components(level, members=True), b0.components(level, members=True)
            for f in c0:
                assert np.array_equal(c[f], c0[f]), f
        nb, nb0 = b.neighbors(3), b0.neighbors(3)
        for f in nb0:
            assert np.array_equal(nb[f], nb0[f]), f
    finally:
        b.close()
        b0.close()


def test_all_singletons(engine):
    seqs = planted()["seqs"] + [b""]
    h, near, st = run_grouped(engine, seqs, np.arange(len(seqs)) - 100, 5)
    assert len(h["partner"]) == 0 and not h["rowOffsets"].any() and len(h["rowOffsets"]) == len(seqs) + 1
    assert st["word_steps"] == 0 and st["cells"] == 0 and st["path"] == 0 and st["scan_launches"] == 0
    for f in NEAR:
        assert np.all(near[f] == -1)


@pytest.mark.parametrize("case", ["big_group", "scattered"])
def test_cut_ranges_and_distant_ranges(engine, case):
    """the 1,500 + singletons and the scattered 200-base cases of the host program against the reference: a sample of at
    most 20,000 same-group pairs -- random ones, the planted 200 / 201-base pairs always, and up to 5,000 of the pairs the
    batch lists, so that a false hit cannot hide outside the sample"""
    seqs, groups = SG.big_group_case() if case == "big_group" else SG.scattered_case()
    k, n = 2, len(seqs)
    h, near, st = run_grouped(engine, seqs, groups, k)
    lens = [len(s) for s in seqs]
    assert st["cells"] == SG.grouped_cells(lens, groups) and st["word_steps"] == SG.grouped_word_steps(lens, groups, k)
    first, second = SG.same_group_pairs(groups)
    rng = np.random.default_rng(3)
    pick = np.zeros(len(first), dtype=bool)
    pick[rng.choice(len(first), size=min(15_000, len(first)), replace=False)] = True
    long = (np.array(lens)[first] >= 200) & (np.array(lens)[second] >= 200)   # the planted 200 / 201-base pairs
    pick |= long
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    code = first * n + second
    hit_at = np.searchsorted(code, row.astype(np.int64) * n + h["partner"])
    assert np.all(hit_at < len(code)) and np.array_equal(code[hit_at], row.astype(np.int64) * n + h["partner"])   # same-group pairs only
    pick[hit_at[:5_000]] = True
    assert pick.sum() <= 20_000
    ed = ref_pairs(seqs, first[pick], second[pick], k)
    got = np.full(len(first), -1, dtype=np.int32)
    got[hit_at] = h["editDistance"]
    bad = np.flatnonzero(got[pick] != ed)
    assert len(bad) == 0, (case, first[pick][bad[:5]], second[pick][bad[:5]], got[pick][bad[:5]], ed[bad[:5]])
    if case == "scattered":
        assert long.sum() == 3 and np.all(got[long] == 1)
    else:
        assert len(h["partner"]) > 10_000


def test_off_kernel_routes(engine):
    rng = np.random.default_rng(17)
    long = SG._rand(rng, 300)
    seqs = [SG._rand(rng, 30) for _ in range(12)]
    groups = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    seqs += [long, long[:150] + b"T" + long[150:], long, b"", b"", b"", seqs[4][:29] + b"A", b""]
    groups += [0, 0, 1, 2, 2, 1, 1, 5]
    # 12, 13: a 300-base pair inside group 0; 14: 300 bases in group 1 (identical to 12: no hit across groups);
    # 15, 16: two empties in group 2 (one distance-0 hit; against its 30-base members: 30 whatever k);
    # 17: an empty in group 1 (30, 30, 30, 30, 30 and 300); 19: an empty alone in group 5
    groups = np.array(groups)
    h, st, (first, second, ed) = assert_grouped(engine, seqs, groups, 1)
    assert st["path"] == (8 | 2)
    pairs = dict(zip(zip(first.tolist(), second.tolist()), ed.tolist()))
    assert pairs[(12, 13)] == 1 and pairs[(15, 16)] == 0 and pairs[(8, 15)] == 30 and pairs[(14, 17)] == 300
    row = np.repeat(np.arange(len(seqs)), np.diff(h["rowOffsets"]))
    listed = dict(zip(zip(row.tolist(), h["partner"].tolist()), h["editDistance"].tolist()))
    assert listed[(12, 13)] == 1 and listed[(15, 16)] == 0 and listed[(4, 17)] == 30 and listed[(14, 17)] == 300
    assert (12, 14) not in listed and (15, 17) not in listed and not any(19 in p for p in listed)
    # only empties and short ones: the kernel and the host, no pair batch
    _, st, _ = assert_grouped(engine, seqs[:12] + [b"", b""], np.array(groups[:12].tolist() + [0, 0]), 1)
    assert st["path"] == 8
    # 17 symbols: every same-group pair through the pair batch, none on the kernel
    wide = [bytes(rng.choice(np.frombuffer(b"ABCDEFGHIJKLMNOPQ", dtype=np.uint8), size=int(m))) for m in rng.integers(20, 30, size=40)]
    wide[5] = wide[6] = wide[3]                                            # 3 and 6 share a group, 5 is in another
    wgroups = np.arange(40) % 3
    assert len(set(b"".join(wide))) == 17
    h, st, _ = assert_grouped(engine, wide, wgroups, 3, word_steps=False)
    assert st["path"] == 2 and st["word_steps"] == 0
    row = np.repeat(np.arange(40), np.diff(h["rowOffsets"]))
    listed = dict(zip(zip(row.tolist(), h["partner"].tolist()), h["editDistance"].tolist()))
    assert listed[(3, 6)] == 0 and (3, 5) not in listed and (5, 6) not in listed


@pytest.mark.parametrize("num_groups", [100_000, 200_000])
def test_many_small_groups(engine, num_groups):
    """12 bp in groups of 3, k = 1, all pairs against the reference.  200,000 groups are 75,000 query tiles of eight slots,
    more than 65,535 work items in one launch (tests/self_groups_host.cpp counts them for this shape)."""
    rng = np.random.default_rng(23)
    n = 3 * num_groups
    founders = rng.integers(0, 4, size=(num_groups, 12))
    codes = np.repeat(founders, 3, axis=0)
    change = rng.random(n) < 0.5                                               # half of them one substitution away
    codes[change, rng.integers(0, 12, size=int(change.sum()))] = rng.integers(0, 4, size=int(change.sum()))
    order = rng.permutation(n)                                                 # no group is contiguous
    codes, groups = codes[order], (np.repeat(np.arange(num_groups), 3) - 7)[order]
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]                       # [n, 12] uint8
    b = engine.SelfBatch(seqs, k=1, hits=True, groups=groups)
    try:
        st = b.run()
        h = b.hits()
    finally:
        b.close()
    first, second = SG.same_group_pairs(groups)
    assert len(first) == n
    ed = ref_pairs(seqs, first, second, 1)
    assert_csr(h, n, SG.csr_of_pairs(n, first, second, ed))
    assert st["cells"] == n * 144 and st["word_steps"] == n * 12 and st["scan_launches"] == 1
    assert 0.3 * n < len(h["partner"]) < n


def _union_find_labels(n, a, b):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    return np.array([find(x) for x in range(n)], dtype=np.int32)


def test_downstream_views(engine):
    p = planted()
    seqs, groups = p["seqs"], p["groups"]
    n, k = len(seqs), 5
    first, second, ed = ref_grouped(seqs, groups, k)
    b = engine.SelfBatch(seqs, k=k, hits=True, groups=groups)
    pb = engine.PairBatch([], [], mode="NW", task="path")
    twin = engine.PairBatch([], [], mode="NW", task="path")
    try:
        b.run()
        for level in (2, 5):
            keep = (ed >= 0) & (ed <= level)
            want = _union_find_labels(n, first[keep], second[keep])
            got = b.components(level, members=True)
            assert np.array_equal(got["label"], want)
            assert np.all(groups[got["label"]] == groups)                      # no component spans two groups
            model = engine.self_components_model(n, *[b.hits()[f] for f in ("rowOffsets", "partner", "editDistance")], level)
            for f in model:
                assert np.array_equal(got[f], model[f]), f
        assert np.array_equal(engine.cluster_within(seqs, 2, groups=groups), b.components(2)["label"])
        nb = b.neighbors(3)
        want = engine.neighbors_model(n, np.concatenate([first, second]), np.concatenate([second, first]),
                                      np.concatenate([ed, ed]), 3, -1)
        for f in want:
            assert np.array_equal(nb[f], want[f]), f
        knn = engine.knn(seqs, 3, k, groups=groups)
        for f in want:
            assert np.array_equal(knn[f], want[f]), f
        h = b.hits()
        row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
        pb.set_cells(b, row, h["partner"])
        pb.run()
        twin.set_pairs([seqs[int(i)] for i in row], [seqs[int(j)] for j in h["partner"]])
        twin.run()
        got, want = pb.results_flat(), twin.results_flat()
        for f in want:
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(got["editDistance"], h["editDistance"])
        for x, y in zip(pb.cigars(), twin.cigars()):
            assert np.array_equal(x, y)
    finally:
        b.close()
        pb.close()
        twin.close()


def test_refused_create_and_dense_views(engine):
    import ctypes as C
    seqs = planted()["seqs"][:8]
    L = engine.lib()
    sd, so = engine._pack(seqs)
    g = np.zeros(8, dtype=np.int32)
    # refused before the device is looked at: the reason is the argument's even on a device that does not exist, so
    # nothing was allocated; the error stays set
    for device in (0, 4096):
        cfg, keep = engine._make_config("NW", "distance", 1, None)
        assert not L.edlibAmdBatchCreateSelfHitsGrouped(sd.ctypes.data, so.ctypes.data, 8, None, cfg, device)
        assert "groups is NULL" in engine.last_error() and "edlibAmdBatchCreateSelfHits" in engine.last_error()
        cfg, keep = engine._make_config("NW", "distance", -1, None)
        assert not L.edlibAmdBatchCreateSelfHitsGrouped(sd.ctypes.data, so.ctypes.data, 8, g.ctypes.data, cfg, device)
        assert "config.k >= 0" in engine.last_error()
    cfg, keep = engine._make_config("NW", "distance", 1, None)
    assert not L.edlibAmdBatchCreateSelfHitsGrouped(sd.ctypes.data, so.ctypes.data, 8, g.ctypes.data, cfg, 4096)
    assert "device 4096 out of range" in engine.last_error()
    b = engine.SelfBatch(seqs, k=1, hits=True, groups=[0, 1] * 4)
    try:
        b.run()
        with pytest.raises(RuntimeError, match="grouped self batch keeps no condensed vector"):
            b.condensed()
        v = engine.SelfView()
        assert L.edlibAmdBatchSelfView(b._h, engine.SELF_DISTANCES | engine.SELF_NEAREST, C.byref(v)) == 0
        assert not v.editDistance and v.numPairs == 2 * 6 and v.numSequences == 8
        with pytest.raises(RuntimeError, match="both-strand"):
            b.strands()
        with pytest.raises(RuntimeError):
            b.results()
    finally:
        b.close()
