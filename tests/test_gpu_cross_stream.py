"""GPU: streamed targets (edlibAmdBatchCrossSetTargets, CrossBatch.set_targets): a resident cross batch whose target set
is replaced must be, after its next run(), exactly a fresh batch created over (its queries, the new targets) -- every
array of every view and the statistics that describe the work -- for every kind of cross batch, through changes of the
tile shape, the alphabet and the empty set; a refused set must leave the batch as it was."""
import numpy as np
import pytest

from test_gpu_cross import IUPAC, _rand, check_cells, ref_cells

pytestmark = pytest.mark.gpu

KINDS = {
    "dense": dict(k=-1),
    "hits": dict(hits=True, k=3),
    "occurrences": dict(occurrences=True, k=2),
    "dense_both": dict(strands="both", k=3),
    "hits_both": dict(hits=True, strands="both", k=3),
}
STATS = ("cells", "word_steps", "path", "scan_launches")
QLENS = [0, 1, 2, 3, 5, 8, 24, 31, 32, 33, 63, 64, 65, 128, 255, 256]


def _queries(rng, alpha, targets=(), n=40):
    """n queries of 0..256 bases; every third one is cut from a target (cells within a small k)."""
    lens = QLENS + [int(x) for x in rng.integers(1, 257, size=n - len(QLENS))]
    out = []
    for i, m in enumerate(lens):
        src = [t for t in targets if len(t) >= m]
        if i % 3 == 0 and m > 0 and src:
            t = src[int(rng.integers(0, len(src)))]
            s = int(rng.integers(0, len(t) - m + 1))
            out.append(t[s:s + m])
        else:
            out.append(_rand(rng, m, alpha))
    return out


def _targets(rng, alpha, nt, lens=()):
    lens = list(lens)[:nt]
    lens += [int(x) for x in rng.integers(0, 301, size=nt - len(lens))]
    return [_rand(rng, n, alpha) for n in lens]


def _views(b):
    """Every array of every view the batch's kind has, as {name: array}."""
    out = {}
    if b.is_occurrences:
        out.update(("occurrences." + f, v) for f, v in b.occurrences().items())
        return out
    if b.is_hits:
        out.update(("hits." + f, v) for f, v in b.hits().items())
    else:
        out.update(("matrix." + f, v) for f, v in b.matrix().items())
    out.update(("best." + f, v) for f, v in b.best().items())
    if b.both_strands:
        out.update(("strands." + f, v) for f, v in b.strands().items())
    return out


def _same(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for f in want:
        assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())


def _fresh(engine, queries, targets, mode, eqs=None, **kind):
    b = engine.CrossBatch(queries, targets, mode=mode, additionalEqualities=eqs, **kind)
    try:
        st = b.run()
        return _views(b), st
    finally:
        b.close()


def _check_hits(h, queries, targets, mode, k, eqs=None):
    """every hit of a hits() list against the checker"""
    n = len(h["query"])
    if n == 0:
        return
    t_ = np.searchsorted(h["targetOffsets"], np.arange(n), side="right") - 1
    ed, nloc, first = ref_cells(queries, targets, mode, k, eqs, [(int(t), int(q)) for t, q in zip(t_, h["query"])])
    assert np.array_equal(h["editDistance"], ed)
    assert np.array_equal(h["numLocations"], nloc)
    assert np.array_equal(h["endLocation"], first)


def _stream_and_compare(engine, b, queries, targets, mode, kind, eqs=None, what=""):
    """set_targets + run on b against a fresh batch: views, statistics, and the forward kinds against the checker"""
    b.set_targets(targets)
    assert b.numTargets == len(targets) and b.n == len(queries) * len(targets)
    st = b.run()
    got = _views(b)
    want, wst = _fresh(engine, queries, targets, mode, eqs, **kind)
    _same(got, want, what)
    assert {f: st[f] for f in STATS} == {f: wst[f] for f in STATS}, what
    if not b.both_strands and not b.is_occurrences:
        if b.is_hits:
            _check_hits(b.hits(), queries, targets, mode, kind["k"], eqs)
        else:
            check_cells(b, queries, targets, mode, kind["k"], eqs)
    return got


# (occurrence batches are HW only)
@pytest.mark.parametrize("kind,mode", [(kind, mode) for kind in sorted(KINDS) for mode in ("NW", "SHW", "HW")
                                       if kind != "occurrences" or mode == "HW"])
def test_stream_equals_fresh_batch(engine, checker, kind, mode):
    rng = np.random.default_rng(sorted(KINDS).index(kind) * 10 + ["NW", "SHW", "HW"].index(mode))
    a = _targets(rng, b"ACGT", 90)
    bset = _targets(rng, b"ACGT", 130, lens=[0, 1, 7, 8, 9, 300])
    queries = _queries(rng, b"ACGT", bset)
    b = engine.CrossBatch(queries, a, mode=mode, **KINDS[kind])
    try:
        b.run()
        _views(b)
        _stream_and_compare(engine, b, queries, bset, mode, KINDS[kind], what=(kind, mode))
    finally:
        b.close()


def _set_targets_raw(b, targets, lead=0, offsets=None):
    """edlibAmdBatchCrossSetTargets on the handle itself: `lead` bytes in front of the pool (offsets that do not start
    at 0), or offsets of the caller's own.  Returns the status; on success the Python side's counts follow."""
    import edlib_amd
    pool = np.frombuffer(b"#" * lead + b"".join(targets) + b"\0", dtype=np.uint8)
    if offsets is None:
        offsets = np.zeros(len(targets) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(t) for t in targets])
        offsets += lead
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rc = edlib_amd.lib().edlibAmdBatchCrossSetTargets(b._h, pool.ctypes.data, offsets.ctypes.data, len(offsets) - 1)
    if rc == 0 and hasattr(b, "numTargets"):
        b.numTargets = len(offsets) - 1
        b.n = b.numQueries * b.numTargets
    return rc


def test_stream_shapes(engine, checker):
    """nt 7 -> 130 -> 1 -> 0 -> 65 on one batch (the tile width, partial tiles, the empty set), the lengths at the pack's
    dword boundary, one target of exactly 65,536 bases, offsets that do not start at 0"""
    rng = np.random.default_rng(77)
    queries = _queries(rng, b"ACGT")
    kind = KINDS["dense"]
    first = _targets(rng, b"ACGT", 7, lens=[0, 1, 7, 8, 9])
    b = engine.CrossBatch(queries, first, mode="HW", **kind)
    try:
        b.run()
        check_cells(b, queries, first, "HW", -1)
        for nt, lens in ((130, [65536, 0, 1, 7, 8, 9, 15, 16, 17]), (1, [9]), (0, []), (65, [8, 0, 7])):
            ts = _targets(rng, b"ACGT", nt, lens=lens)
            _stream_and_compare(engine, b, queries, ts, "HW", kind, what=nt)
        # the same through offsets that start at 11
        ts = _targets(rng, b"ACGT", 33, lens=[9, 8, 7, 1, 0])
        assert _set_targets_raw(b, ts, lead=11) == 0, engine.last_error()
        b.run()
        _same(_views(b), _fresh(engine, queries, ts, "HW", **kind)[0], "lead")
        check_cells(b, queries, ts, "HW", -1)
    finally:
        b.close()


TWELVE = b"ACDEFGHIKLMN"


@pytest.mark.parametrize("kind", ["dense", "hits"])
def test_stream_alphabets(engine, checker, kind):
    """ACGT -> ACGTN -> 12 symbols -> ACGT: the Peq rows per word go 4 -> 8 -> 16 -> 4 on one batch"""
    rng = np.random.default_rng(5 + len(kind))
    sets = [_targets(rng, alpha, 40) for alpha in (b"ACGT", b"ACGTN", TWELVE, b"ACGT")]
    queries = (_queries(rng, b"ACGT", sets[0], n=20) + _queries(rng, b"ACGTN", sets[1], n=20) +
               _queries(rng, TWELVE, sets[2], n=20))
    b = engine.CrossBatch(queries, sets[0], mode="HW", **KINDS[kind])
    try:
        b.run()
        for i, ts in enumerate(sets[1:]):
            _stream_and_compare(engine, b, queries, ts, "HW", KINDS[kind], what=(kind, i))
    finally:
        b.close()


def test_stream_with_equalities(engine, checker):
    rng = np.random.default_rng(9)
    a = _targets(rng, b"ACGT", 30)
    ts = _targets(rng, b"ACGTRYN", 50)
    queries = _queries(rng, b"ACGTRYN", ts)
    kind = dict(k=3)
    b = engine.CrossBatch(queries, a, mode="HW", additionalEqualities=IUPAC, **kind)
    try:
        b.run()
        _stream_and_compare(engine, b, queries, ts, "HW", kind, eqs=IUPAC, what="iupac")
    finally:
        b.close()


@pytest.mark.parametrize("kind", ["hits", "dense_both"])
def test_stream_leaves_no_stale_state(engine, kind):
    rng = np.random.default_rng(31 + len(kind))
    a = _targets(rng, b"ACGT", 100)
    bset = _targets(rng, b"ACGTN", 37)
    queries = _queries(rng, b"ACGT", a)
    b = engine.CrossBatch(queries, a, mode="HW", **KINDS[kind])
    try:
        s1 = b.run()
        v1 = _views(b)
        b.set_targets(bset)
        b.run()
        _views(b)
        b.set_targets(a)
        s2 = b.run()
        _same(_views(b), v1, kind)
        assert {f: s1[f] for f in STATS} == {f: s2[f] for f in STATS}
    finally:
        b.close()


def test_stream_keeps_the_grown_hit_list(engine):
    """1,024 x 1,100 identical 20-mers at k = 0: 1,126,400 hits, past the 2^20 the list starts at.  The Run that finds
    that out grows the list and scans again; the next set of the same size fits and scans once."""
    seq, other = b"ACGTTGCAACGTACGTTGCA", b"TTGCAACGTACGTTGCAACG"
    nq, nt = 1024, 1100
    b = engine.CrossBatch([seq] * nq, [seq] * nt, mode="NW", k=0, hits=True)
    try:
        st = b.run()
        assert st["scan_launches"] == 2, st
        assert len(b.hits()["query"]) == nq * nt > 1 << 20
        b.set_targets([other] * (nt - 1) + [seq])
        st = b.run()
        assert st["scan_launches"] == 1, st
        h = b.hits()
        assert h["targetOffsets"].tolist() == [0] * nt + [nq]
        assert np.array_equal(h["query"], np.arange(nq)) and not h["editDistance"].any()
        b.set_targets([seq] * nt)
        st = b.run()
        assert st["scan_launches"] == 1, st
        h = b.hits()
        assert np.array_equal(h["targetOffsets"], np.arange(nt + 1) * nq)
        assert np.array_equal(h["query"], np.tile(np.arange(nq), nt)) and not h["editDistance"].any()
    finally:
        b.close()


def test_stream_refusals_leave_the_batch_as_it_was(engine):
    rng = np.random.default_rng(13)
    a = _targets(rng, b"ACGT", 50)
    queries = _queries(rng, b"ACGT", a)
    ok = _targets(rng, b"ACGT", 5)
    seventeen = [bytes(range(65, 82)), b"ACG"]
    b = engine.CrossBatch(queries, a, mode="HW", hits=True, k=3)
    try:
        b.run()
        before = _views(b)
        held = b.hits(copy=False)
        for bad, limit in ((ok + [b"A" * 65537], "65,536"), (seventeen, "limit for a streamed set is 16")):
            with pytest.raises(RuntimeError) as e:
                b.set_targets(bad)
            assert limit in str(e.value) and "create a new batch" in str(e.value), str(e.value)
            assert b.numTargets == len(a)
            _same(_views(b), before, limit)
        down = np.array([0, 10, 5, 20], dtype=np.int64)
        assert _set_targets_raw(b, [b"ACGT" * 5], offsets=down) != 0
        assert "offsets" in engine.last_error()
        assert _set_targets_raw(b, ok, offsets=np.zeros(0, dtype=np.int64)) != 0        # numTargets = -1
        assert engine.lib().edlibAmdBatchCrossSetTargets(b._h, None, None, 3) != 0
        assert "NULL" in engine.last_error()
        _same(_views(b), before, "after every refusal")
        _same({f: np.array(v) for f, v in held.items()}, {f: before["hits." + f] for f in held}, "the pinned view")
        b.run()
        _same(_views(b), before, "the next run")
    finally:
        b.close()

    # a batch that holds a 300-base query streams no targets
    long_q = queries[:5] + [_rand(rng, 300, b"ACGT")]
    b = engine.CrossBatch(long_q, a, mode="HW")
    try:
        b.run()
        before = _views(b)
        with pytest.raises(RuntimeError) as e:
            b.set_targets(ok)
        assert "query 5 has 300 bases" in str(e.value) and "256" in str(e.value), str(e.value)
        _same(_views(b), before, "long query")
        b.run()
        _same(_views(b), before, "long query, the next run")
    finally:
        b.close()

    # nor does a self batch
    seqs = [_rand(rng, 20, b"ACGT") for _ in range(30)]
    s = engine.SelfBatch(seqs)
    try:
        s.run()
        before = s.condensed()
        assert _set_targets_raw(s, ok) != 0
        assert "edlibAmdBatchCrossSetTargets" in engine.last_error() and "self batch" in engine.last_error()
        assert np.array_equal(s.condensed(), before)
        s.run()
        assert np.array_equal(s.condensed(), before)
    finally:
        s.close()


@pytest.mark.parametrize("start", ["empty", "sessions"])
def test_stream_into_a_batch_without_kernel_targets(engine, checker, start):
    """a batch created over no targets, and one whose Create sent every target through internal sessions (17 symbols, a
    target above 65,536 bases): the first set_targets finds the queries resident and drops the sessions"""
    rng = np.random.default_rng(41)
    ts = _targets(rng, b"ACGT", 70)
    queries = _queries(rng, b"ACGT", ts)
    first = [] if start == "empty" else [bytes(range(65, 82)) * 3, _rand(rng, 65537, b"ACGT")]
    kind = KINDS["hits"]
    b = engine.CrossBatch(queries, first, mode="HW", **kind)
    try:
        st = b.run()
        assert not st["path"] & 8 and (st["path"] != 0) == (start == "sessions"), st      # bit 3: the cross kernel ran
        _stream_and_compare(engine, b, queries, ts, "HW", kind, what=start)
        assert b.stats()["path"] == 8
    finally:
        b.close()


def test_stream_views_need_a_run(engine):
    rng = np.random.default_rng(3)
    queries = _queries(rng, b"ACGT", n=20)
    b = engine.CrossBatch(queries, _targets(rng, b"ACGT", 10), mode="HW")
    try:
        b.run()
        b.matrix()
        b.set_targets(_targets(rng, b"ACGT", 12))
        for view in (b.matrix, b.best):
            with pytest.raises(RuntimeError, match="Run it first"):
                view()
        b.run()
        assert b.matrix()["editDistance"].shape == (12, len(queries))
    finally:
        b.close()
