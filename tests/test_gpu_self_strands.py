"""GPU: both-strand self batches (edlibAmdBatchCreateSelfBothStrands / CreateSelfHitsBothStrands).  The reference is the
checker on the pairs (seqs[i], seqs[j]) and (reverse_complement(seqs[i]), seqs[j]), i < j, folded by
self_strands_model(); every comparison is exact.  The hit list is compared with the reference's pairs within k, nearest()
with self_nearest_model(), nearestStrand with the pair's byte, the counters with twice the one-strand formulas."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_cross import IUPAC, _pack, _rand
from test_gpu_self import NEAR, assert_csr, assert_nearest, csr_of, mixed, ref_pairs
from test_self_model import self_cells, self_word_steps
from test_self_strands_model import complement_symmetric

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def ref_rev_pairs(engine, seqs, i, j, k, eqs=None):
    """editDistance of edlibAlign(reverse_complement(seqs[i]), seqs[j], NW, k) for the listed pairs, by the checker."""
    if len(i) == 0:
        return np.zeros(0, dtype=np.int32)
    qp, qo = _pack([engine.reverse_complement(bytes(seqs[int(a)])) for a in i])
    tp, to = _pack([bytes(seqs[int(b)]) for b in j])
    r = O.pool_align(qp, qo, tp, to, False, "NW", "distance", k, eq_pairs=eqs)
    return np.asarray(r["editDistance"]).astype(np.int32)


def ref_both(engine, seqs, k, eqs=None, i=None, j=None):
    """(combined distances, strand bytes) of the pairs i < j (all of them by default): the definition by index."""
    if i is None:
        i, j = np.triu_indices(len(seqs), 1)
    return engine.self_strands_model(ref_pairs(seqs, i, j, k, eqs), ref_rev_pairs(engine, seqs, i, j, k, eqs))


def run_dense(engine, seqs, k, eqs=None):
    b = engine.SelfBatch(seqs, k=k, additionalEqualities=eqs, strands="both")
    try:
        st = b.run()
        return b.condensed(), b.strands(), b.nearest(), st
    finally:
        b.close()


def run_hits(engine, seqs, k, eqs=None):
    b = engine.SelfBatch(seqs, k=k, additionalEqualities=eqs, hits=True, strands="both")
    try:
        st = b.run()
        return b.hits(), b.strands(), b.nearest(), st
    finally:
        b.close()


def assert_nearest_strand(engine, n, near, nearest_strand, pair_strand):
    """nearestStrand[x] is the byte of the pair (x, nearest[x]), 0 where there is none; pair_strand is condensed."""
    assert nearest_strand.dtype == np.uint8 and nearest_strand.shape == (n,)
    x = np.arange(n)
    has = near["nearest"] >= 0
    want = np.zeros(n, dtype=np.uint8)
    if has.any():
        want[has] = pair_strand[engine.condensed_index(n, x[has], near["nearest"][has])]
    bad = np.nonzero(nearest_strand != want)[0]
    assert len(bad) == 0, (bad[:5], nearest_strand[bad[:5]], want[bad[:5]])


def assert_counters(st, seqs, k, kernel=True):
    lens = [len(s) for s in seqs]
    assert st["cells"] == 2 * self_cells(lens)
    if kernel:
        assert st["word_steps"] == 2 * self_word_steps(lens, k)


def assert_dense(engine, seqs, k, want, eqs=None, kernel=True):
    """want = (distances, strand bytes), condensed"""
    cond, s, near, st = run_dense(engine, seqs, k, eqs)
    n = len(seqs)
    i, j = np.triu_indices(n, 1)
    assert cond.dtype == np.int32 and cond.shape == want[0].shape
    bad = np.nonzero(cond != want[0])[0]
    assert len(bad) == 0, (k, [(int(i[b]), int(j[b]), int(cond[b]), int(want[0][b])) for b in bad[:5]])
    ps = s["pairStrand"]
    assert ps.dtype == np.uint8 and ps.shape == want[1].shape
    bad = np.nonzero(ps != want[1])[0]
    assert len(bad) == 0, (k, [(int(i[b]), int(j[b]), int(ps[b]), int(want[1][b])) for b in bad[:5]])
    assert_nearest(engine, near, n, want[0])
    assert_nearest_strand(engine, n, near, s["nearestStrand"], want[1])
    assert_counters(st, seqs, k, kernel)
    return cond, ps, st


def assert_hits(engine, seqs, k, want, eqs=None, kernel=True):
    h, s, near, st = run_hits(engine, seqs, k, eqs)
    n = len(seqs)
    assert_csr(h, n, csr_of(n, want[0]))
    hs = s["hitStrand"]
    assert hs.dtype == np.uint8
    assert np.array_equal(hs, want[1][want[0] != -1])
    assert_nearest(engine, near, n, want[0])
    assert_nearest_strand(engine, n, near, s["nearestStrand"], want[1])
    assert_counters(st, seqs, k, kernel)
    return h, hs, st


def flip_some(engine, seqs, every, start=0):
    return [engine.reverse_complement(s) if x % every == start else s for x, s in enumerate(seqs)]


_MIXED = {}


def mixed_both(engine):
    """The 200-sequence mixed() set with every third sequence reverse-complemented, and its reference, computed once."""
    if not _MIXED:
        seqs = flip_some(engine, mixed()[0], 3)
        _MIXED["seqs"] = seqs
        _MIXED["ref"] = {k: ref_both(engine, seqs, k) for k in (-1, 0, 3)}
    return _MIXED["seqs"], _MIXED["ref"]


@pytest.mark.parametrize("k", [-1, 3])
def test_self_strands_mixed_dense(engine, checker, k):
    seqs, ref = mixed_both(engine)
    assert len(seqs) == 200 and complement_symmetric(b"".join(seqs))
    _, ps, st = assert_dense(engine, seqs, k, ref[k])
    assert st["path"] & 8 and st["scan_launches"] == 3
    assert np.any(ps & 1) and np.any(ps & 2)


@pytest.mark.parametrize("k", [0, 3])
def test_self_strands_mixed_hits(engine, checker, k):
    seqs, ref = mixed_both(engine)
    h, hs, st = assert_hits(engine, seqs, k, ref[k])
    assert st["path"] & 8
    assert len(h["partner"]) >= 2 * 198 - 1                        # every pair with an empty sequence
    assert np.any(hs & 1) and np.any(hs & 2)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 64, 65, 129])
def test_self_strands_tile_edges(engine, checker, n):
    """Tiles of 32 sequences at a boundary, odd counts and padding mate pairs; one planted reverse-complement duplicate."""
    rng = np.random.default_rng(100 + n)
    arr = rng.choice(ACGT, size=(n, 24)).astype(np.uint8)
    seqs = [bytes(r) for r in arr]
    seqs[n // 2] = engine.reverse_complement(seqs[0]) if n > 1 else seqs[0]
    want = ref_both(engine, seqs, 8)
    cond, ps, st = assert_dense(engine, seqs, 8, want)
    assert st["word_steps"] == 2 * (n * (n - 1) // 2) * 24
    if n > 1:
        at = engine.condensed_index(n, 0, n // 2)
        assert cond[at] == 0 and ps[at] == 1                        # the planted duplicate, found in reverse only
    assert_hits(engine, seqs, 8, want)
    if n == 64:
        c = engine.CrossBatch(seqs, seqs, "NW", k=8, strands="both")
        try:
            cst = c.run()
            m = c.matrix()["editDistance"]
            cs = c.strands()["cellStrand"]
        finally:
            c.close()
        i, j = np.triu_indices(n, 1)
        assert np.array_equal(m[j, i], cond)                       # cell (query i, target j)
        assert np.array_equal(cs[j, i], ps)
        assert 2 * st["word_steps"] + 2 * 64 * 24 == cst["word_steps"]


def test_self_strands_work_items(engine, checker):
    """4,096 sequences in 64 families, half of each reverse-complemented: query tiles of 32 sequences whose ranges are cut
    into several work items each."""
    rng = np.random.default_rng(11)
    arr = np.repeat(rng.choice(ACGT, size=(64, 32)).astype(np.uint8), 64, axis=0)
    for _ in range(2):
        pos = rng.integers(0, 32, size=len(arr))
        arr[np.arange(len(arr)), pos] = rng.choice(ACGT, size=len(arr))
    seqs = flip_some(engine, [bytes(r) for r in arr], 2)
    seqs = [seqs[int(o)] for o in rng.permutation(len(seqs))]
    n = len(seqs)
    h, s, near, st = run_hits(engine, seqs, 2)
    c = engine.CrossBatch(seqs, seqs, "NW", k=2, hits=True, strands="both")
    try:
        cst = c.run()
        ch = c.hits()
        chs = c.strands()["hitStrand"]
    finally:
        c.close()
    t = np.repeat(np.arange(n), np.diff(ch["targetOffsets"]))
    q = ch["query"].astype(np.int64)
    up = q < t                                                      # query i (either strand) against target j, i < j
    order = np.lexsort((t[up], q[up]))
    want = {"rowOffsets": np.concatenate([[0], np.cumsum(np.bincount(q[up], minlength=n))]).astype(np.int64),
            "partner": t[up][order].astype(np.int32), "editDistance": ch["editDistance"][up][order]}
    assert_csr(h, n, want)
    assert np.array_equal(s["hitStrand"], chs[up][order])
    assert np.any(s["hitStrand"] & 1) and np.any(s["hitStrand"] == 0)
    assert st["word_steps"] == 2 * (n * (n - 1) // 2) * 32 and 2 * st["word_steps"] + 2 * n * 32 == cst["word_steps"]
    assert st["word_steps"] < 0.60 * cst["word_steps"]
    # 2,000 sampled pairs against the checker: half of them hits, half anywhere in the triangle
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    pick = rng.choice(len(row), size=1000, replace=False)
    we, ws = ref_both(engine, seqs, 2, i=row[pick], j=h["partner"][pick])
    assert np.array_equal(we, h["editDistance"][pick]) and np.array_equal(ws, s["hitStrand"][pick])
    i = rng.integers(0, n - 1, size=1000)
    j = np.minimum(i + 1 + rng.integers(0, n, size=1000) % (n - 1 - i), n - 1)
    got, gots = np.full(1000, -1, dtype=np.int32), np.zeros(1000, dtype=np.uint8)
    keys = row.astype(np.int64) * n + h["partner"]
    at = np.searchsorted(keys, i * n + j)
    found = (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == i * n + j)
    got[found] = h["editDistance"][at[found]]
    gots[found] = s["hitStrand"][at[found]]
    we, ws = ref_both(engine, seqs, 2, i=i, j=j)
    assert np.array_equal(we, got) and np.array_equal(ws, gots)
    want_near = engine.self_nearest_model(n, row, h["partner"], h["editDistance"])
    for f in NEAR:
        assert np.array_equal(near[f], want_near[f]), f
    has = near["nearest"] >= 0
    x = np.arange(n)[has]
    p = near["nearest"][has].astype(np.int64)
    hit_at = np.searchsorted(keys, np.minimum(x, p) * n + np.maximum(x, p))
    assert np.array_equal(s["nearestStrand"][has], s["hitStrand"][hit_at]) and not s["nearestStrand"][~has].any()


def test_self_strands_length_window(engine, checker):
    rng = np.random.default_rng(13)
    base = _rand(rng, 60, b"ACGT")
    seqs = []
    for m in rng.integers(20, 61, size=300):
        s = bytearray(base[:int(m)])
        for p in rng.integers(0, int(m), size=int(rng.integers(0, 3))):
            s[int(p)] = b"ACGT"[int(rng.integers(0, 4))]
        seqs.append(bytes(s))
    seqs = flip_some(engine, seqs, 2, 1)
    want = ref_both(engine, seqs, 2)
    lens = np.array([len(s) for s in seqs])
    i, j = np.triu_indices(len(seqs), 1)
    outside = np.abs(lens[i] - lens[j]) > 2
    assert np.all(want[0][outside] == -1) and not want[1][outside].any() and np.count_nonzero(want[0] != -1) > 300
    _, ps, st = assert_dense(engine, seqs, 2, want)
    assert np.any(ps & 1)
    lo, hi = np.minimum(lens[i], lens[j]), np.maximum(lens[i], lens[j])
    assert st["word_steps"] == 2 * int((((lo + 31) // 32) * hi)[~outside].sum())
    assert_hits(engine, seqs, 2, want)


def _family(engine, rng, chars, count, flip_every=2):
    base = _rand(rng, 70, chars)
    seqs = []
    for m in rng.integers(5, 71, size=count):
        s = bytearray(base[:int(m)])
        for p in rng.integers(0, int(m), size=2):
            s[int(p)] = chars[int(rng.integers(0, len(chars)))]
        seqs.append(bytes(s))
    return flip_some(engine, seqs, flip_every)


@pytest.mark.parametrize("alpha", ["ACGTN", "IUPAC"])
def test_self_strands_kernel_alphabets(engine, checker, alpha):
    chars, eqs = (b"ACGTN", None) if alpha == "ACGTN" else (b"ACGTRYN", IUPAC)
    rng = np.random.default_rng(len(alpha))
    seqs = _family(engine, rng, chars, 80)
    assert complement_symmetric(b"".join(seqs), eqs)
    for k in (-1, 4):
        want = ref_both(engine, seqs, k, eqs)
        _, ps, st = assert_dense(engine, seqs, k, want, eqs)
        assert st["path"] & 8
        assert np.any(ps & 1)
    assert_hits(engine, seqs, 4, want, eqs)


def test_self_strands_with_u_take_the_pair_batch(engine, checker):
    """c(U) = A and c(A) = T: the condition fails, every pair goes through the pair batch in index order."""
    rng = np.random.default_rng(21)
    seqs = _family(engine, rng, b"ACGU", 40)
    assert not complement_symmetric(b"".join(seqs))
    for k in (-1, 4):
        want = ref_both(engine, seqs, k)
        _, _, st = assert_dense(engine, seqs, k, want, kernel=False)
        assert not (st["path"] & 8) and st["path"] & 2 and st["word_steps"] == 0
    _, _, st = assert_hits(engine, seqs, 4, want, kernel=False)
    assert not (st["path"] & 8) and st["path"] & 2


def test_self_strands_unclosed_equalities_take_the_pair_batch(engine, checker):
    """(R, A) without (Y, T): NW(rc(s_i), s_j) and NW(rc(s_j), s_i) differ, so only the index order is right."""
    eqs = [("R", "A")]
    rng = np.random.default_rng(22)
    seqs = [b"RRRRRRRR", b"TTTTTTTT"] + _family(engine, rng, b"ACGTR", 30)
    assert not complement_symmetric(b"".join(seqs), eqs)
    # the case is not vacuous: rc(s_0) = YYYYYYYY matches nothing of s_1, rc(s_1) = AAAAAAAA matches every R of s_0
    a = ref_rev_pairs(engine, seqs, [0], [1], -1, eqs)
    b = ref_rev_pairs(engine, [seqs[1], seqs[0]], [0], [1], -1, eqs)
    assert a[0] == 8 and b[0] == 0
    for k in (-1, 4):
        want = ref_both(engine, seqs, k, eqs)
        cond, _, st = assert_dense(engine, seqs, k, want, eqs, kernel=False)
        assert not (st["path"] & 8) and st["path"] & 2
        assert cond[0] == (8 if k < 0 else -1)
    assert_hits(engine, seqs, 4, want, eqs, kernel=False)


def test_self_strands_other_routes(engine, checker):
    rng = np.random.default_rng(17)
    seqs = [_rand(rng, int(m), b"ACGT") for m in rng.integers(1, 200, size=36)]
    long_ = _rand(rng, 300, b"ACGT")
    seqs[5], seqs[20] = long_, engine.reverse_complement(long_[:150] + b"T" + long_[150:299])
    seqs += [_rand(rng, 300, b"ACGT"), b"", b"", engine.reverse_complement(seqs[7])]
    assert len(seqs) == 40 and sum(1 for s in seqs if len(s) == 300) == 3
    n = len(seqs)
    for k in (-1, 5):
        want = ref_both(engine, seqs, k)
        cond, ps, st = assert_dense(engine, seqs, k, want)
        assert st["path"] & 8 and st["path"] & 2                    # the kernel and the internal pair batch
        at = engine.condensed_index(n, 5, 20)
        assert 0 < cond[at] <= 2 and ps[at] == 1                    # the planted pair, by the pair batch
        assert cond[engine.condensed_index(n, 7, 39)] == 0 and ps[engine.condensed_index(n, 7, 39)] & 1
        assert cond[engine.condensed_index(n, 37, 38)] == 0 and ps[engine.condensed_index(n, 37, 38)] == 2   # two empty
        assert ps[engine.condensed_index(n, 0, 37)] == 2 and cond[engine.condensed_index(n, 0, 37)] == len(seqs[0])
    h, hs, st = assert_hits(engine, seqs, 5, want)
    assert st["path"] & 2
    row5 = slice(h["rowOffsets"][5], h["rowOffsets"][6])
    assert 20 in h["partner"][row5] and hs[row5][h["partner"][row5] == 20][0] == 1
    prot = b"ACDEFGHIKLMNPQRST"                                       # 17 symbols: every pair through the pair batch
    seqs = [_rand(rng, int(m), prot) for m in rng.integers(0, 80, size=10)] + [prot, engine.reverse_complement(prot[:-1])]
    for k in (-1, 3):
        want = ref_both(engine, seqs, k)
        cond, ps, st = assert_dense(engine, seqs, k, want, kernel=False)
        assert not (st["path"] & 8) and st["path"] & 2
        assert cond[-1] == 1 and ps[-1] == 1
    assert_hits(engine, seqs, 3, want, kernel=False)


def test_self_strands_hits_capacity_growth(engine):
    """1,500 x 8 bp at k = 8: every pair is a hit, 1,124,250 of them, past the 2^20 the list starts at."""
    rng = np.random.default_rng(23)
    n = 1500
    seqs = [bytes(r) for r in rng.choice(ACGT, size=(n, 8)).astype(np.uint8)]
    cond, ds, dnear, _ = run_dense(engine, seqs, 8)
    h, hs, hnear, _ = run_hits(engine, seqs, 8)
    assert len(h["partner"]) == n * (n - 1) // 2 == 1_124_250 > 1 << 20
    assert not np.any(cond == -1)
    assert_csr(h, n, csr_of(n, cond))
    assert np.array_equal(hs["hitStrand"], ds["pairStrand"]) and np.any(ds["pairStrand"] & 1)
    assert np.array_equal(hs["nearestStrand"], ds["nearestStrand"])
    for f in NEAR:
        assert np.array_equal(hnear[f], dnear[f]), f


def test_self_strands_repeat_and_misuse(engine):
    seqs = [b"ACGTTGCA", b"ACGTTGCC", b"GGCAACGT", b"TTTTTTTT", b""]
    d = engine.SelfBatch(seqs, k=3, strands="both")
    h = engine.SelfBatch(seqs, k=3, hits=True, strands="both")
    one = engine.SelfBatch(seqs, k=3)
    try:
        with pytest.raises(RuntimeError, match="Run"):
            d.strands()
        runs = []
        for _ in range(2):
            d.run()
            h.run()
            runs.append((d.condensed(), d.strands(), d.nearest(), h.hits(), h.strands(), h.nearest()))
        for a, b in zip(runs[0], runs[1]):
            if isinstance(a, dict):
                assert a.keys() == b.keys() and all(np.array_equal(a[f], b[f]) for f in a)
            else:
                assert np.array_equal(a, b)
        at = engine.condensed_index(len(seqs), 1, 2)                       # GGCAACGT is the reverse complement of ACGTTGCC
        assert runs[0][0][at] == 0 and runs[0][1]["pairStrand"][at] == 1
        assert set(runs[0][1]) == {"pairStrand", "nearestStrand"} and set(runs[0][4]) == {"hitStrand", "nearestStrand"}
        assert set(d.strands(pairs=False)) == {"nearestStrand"}
        one.run()
        with pytest.raises(RuntimeError, match="both-strand"):
            one.strands()
        L = engine.lib()
        import ctypes as C
        assert L.edlibAmdBatchSelfStrands(one._h, engine.SELF_NEAREST, C.byref(engine.SelfStrands())) != 0
        assert "not a both-strand self batch" in engine.last_error()
        assert L.edlibAmdBatchSelfStrands(d._h, 4, C.byref(engine.SelfStrands())) != 0
        c = engine.CrossBatch([b"ACGT"], [b"ACGA"], "NW", strands="both")
        c.run()
        assert L.edlibAmdBatchSelfStrands(c._h, engine.SELF_NEAREST, C.byref(engine.SelfStrands())) != 0
        assert "not a self batch" in engine.last_error()
        c.close()
        with pytest.raises(RuntimeError, match="without hits"):
            h.condensed()
        r = engine.pairs_within(seqs, 3, strands="both")
        for f in ("rowOffsets", "partner", "editDistance"):
            assert np.array_equal(r[f], runs[0][3][f]), f
        assert np.array_equal(r["hitStrand"], runs[0][4]["hitStrand"])
        assert np.array_equal(engine.pdist(seqs, k=3, strands="both"), runs[0][0])
    finally:
        d.close()
        h.close()
        one.close()
