"""GPU: streamed units (edlibAmdBatchWindowsSetUnits, WindowBatch.set_units): a resident window batch whose queries and
units are replaced must be, after its next run(), exactly a fresh batch created over (its target, the new queries, the
new units) -- every array of both views and the statistics that describe the work -- and every unit must equal the
checker on the bytes of its window; a refused set must leave the batch as it was."""
import ctypes as C

import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth, window_best_model
from test_gpu_windows import FIELDS, IUPAC, _read_from, check, host_word_steps, ref_units

pytestmark = pytest.mark.gpu

STATS = ("cells", "word_steps", "path", "scan_launches")
QLENS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 128, 255, 256]
WLENS = [0, 1, 7, 8, 9]


def _unit_set(rng, target, nq=40, nu=300, qlens=QLENS, strands=False):
    """nq queries cut from the target (a few substitutions) and nu units: every query named by the first nq units (where
    nu allows), the window lengths of WLENS, windows at the query's locus (distances within a small k) and anywhere,
    every start phase mod 8 and a window that ends at the target's last column.  Returns (queries, uq, us, ul, strand)."""
    T = len(target)
    lens = list(qlens)[:nq] + [int(x) for x in rng.integers(1, 257, size=max(nq - len(qlens), 0))]
    pos = [int(rng.integers(0, T - 300)) for _ in lens]
    queries = [_read_from(target, p, m, rng, 2) for p, m in zip(pos, lens)]
    st = rng.integers(0, 2, size=nu).astype(np.uint8) if strands else None
    if strands:                                          # half of the queries lie on the other strand of their locus
        queries = [edlib_amd.reverse_complement(q) if i % 2 else q for i, q in enumerate(queries)]
    uq, us, ul = np.zeros(nu, dtype=np.int32), np.zeros(nu, dtype=np.int32), np.zeros(nu, dtype=np.int32)
    for u in range(nu):
        q = u % nq if u < nq else int(rng.integers(0, nq))
        m = lens[q]
        kind = u % 4
        if kind == 0:                                    # the locus itself: NW within k too
            s, n = pos[q], m
        elif kind == 1:                                  # around the locus
            s, n = max(pos[q] - 20, 0), m + 40
        elif kind == 2 and u < 8 * len(WLENS) * 4:       # the short lengths at every start phase
            j = u // 4
            n = WLENS[j % len(WLENS)]
            s = 8 * int(rng.integers(0, (T - 16) // 8)) + (j // len(WLENS)) % 8
        else:
            n = int(rng.integers(1, 500))
            s = int(rng.integers(0, T - n + 1))
        uq[u], us[u], ul[u] = q, s, n
    if nu > 3:
        us[3] = T - ul[3]                                # ends at the last column
    return queries, uq, us, ul, st


def _views(b):
    out = {"units." + f: v for f, v in b.units().items()}
    out.update(("best." + f, v) for f, v in b.best().items())
    return out


def _same(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for f in want:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())


def _fresh(engine, queries, target, uq, us, ul, mode, k, eqs=None, st=None):
    b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k, additionalEqualities=eqs, unit_strand=st)
    try:
        stats = b.run()
        return _views(b), stats
    finally:
        b.close()


def _check_stranded(b, queries, target, uq, us, ul, st, mode, k, eqs=None):
    """units() against the checker on reverse_complement() bytes for the strand-1 units, best() against the model"""
    both = []
    for q in queries:
        both += [q, edlib_amd.reverse_complement(q)]
    got = b.units()
    want = ref_units(both, target, 2 * np.asarray(uq, dtype=np.int64) + np.asarray(st, dtype=np.int64), us, ul, mode, k, eqs)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:5])
    best = b.best()
    for f, v in window_best_model(uq, got["editDistance"], len(queries)).items():
        assert np.array_equal(best[f], v), f


def _stream_and_compare(engine, b, queries, target, uq, us, ul, mode, k, eqs=None, st=None, what=""):
    """set_units + run on b against a fresh batch: views, statistics, and every unit against the checker"""
    b.set_units(queries, uq, us, ul, unit_strand=st)
    assert b.numQueries == len(queries) and b.numUnits == len(uq) == b.n
    stats = b.run()
    got = _views(b)
    want, wstats = _fresh(engine, queries, target, uq, us, ul, mode, k, eqs, st)
    _same(got, want, what)
    assert {f: stats[f] for f in STATS} == {f: wstats[f] for f in STATS}, what
    assert stats["word_steps"] == host_word_steps(queries, uq, ul, mode, k), what
    assert stats["path"] == (16 if len(uq) else 0), (what, stats)
    if st is None:
        check(b, queries, target, uq, us, ul, mode, k, eqs)
    else:
        _check_stranded(b, queries, target, uq, us, ul, st, mode, k, eqs)
    return got, stats


# ---- 1. stream equals a fresh batch

@pytest.mark.parametrize("k", [-1, 3])
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_stream_equals_fresh_batch(engine, checker, mode, k):
    target = synth.random_dna(201, 8000)
    rng = np.random.default_rng(["NW", "SHW", "HW"].index(mode) * 10 + k + 1)
    qa, uqa, usa, ula, _ = _unit_set(rng, target, nq=9, nu=70, qlens=[150, 40, 200])
    queries, uq, us, ul, _ = _unit_set(rng, target)
    assert sorted(set(int(s) % 8 for s in us)) == list(range(8))
    assert set(WLENS) <= set(int(n) for n in ul) and len(target) in (us + ul)
    assert set(QLENS) <= set(len(queries[int(q)]) for q in uq)
    b = engine.WindowBatch(qa, target, uqa, usa, ula, mode=mode, k=k)
    try:
        b.run()
        _views(b)
        got, _ = _stream_and_compare(engine, b, queries, target, uq, us, ul, mode, k, what=(mode, k))
        assert (got["units.editDistance"] >= 0).any()
        if k >= 0:
            assert (got["units.editDistance"] == -1).any()
    finally:
        b.close()


# ---- 2. shapes on one batch

def _set_units_raw(b, queries, uq, us, ul, st=None, lead=0, offsets=None, nu=None):
    """edlibAmdBatchWindowsSetUnits on the handle itself: `lead` bytes in front of the pool (offsets that do not start at
    0), offsets of the caller's own, a unit count of the caller's own.  Returns the status; on success the Python side's
    counts follow."""
    pool = np.frombuffer(b"#" * lead + b"".join(queries) + b"\0", dtype=np.uint8)
    if offsets is None:
        offsets = np.zeros(len(queries) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(q) for q in queries])
        offsets += lead
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    arrs = [np.ascontiguousarray(np.append(a, 0), dtype=np.int32) for a in (uq, us, ul)]
    sp = None if st is None else np.ascontiguousarray(np.append(st, 0), dtype=np.uint8)
    nu = len(uq) if nu is None else nu
    rc = edlib_amd.lib().edlibAmdBatchWindowsSetUnits(b._h, pool.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                                      arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                                      None if sp is None else sp.ctypes.data, nu)
    if rc == 0 and hasattr(b, "numUnits"):
        b.numQueries, b.numUnits, b.n = len(offsets) - 1, nu, nu
    return rc


def test_stream_shapes(engine, checker):
    """numUnits 130 -> 1 -> 0 -> 65 -> 193 and numQueries 12 -> 1 -> 0 -> 40 -> 5 on one batch (ragged waves, the empty
    set, buffers that shrink and grow), queries that no unit names, one query named by 200 units, every unit in one word
    group, offsets that do not start at 0"""
    target = synth.random_dna(202, 8000)
    rng = np.random.default_rng(22)
    mode, k = "HW", -1
    qa, uqa, usa, ula, _ = _unit_set(rng, target, nq=12, nu=130)
    b = engine.WindowBatch(qa, target, uqa, usa, ula, mode=mode, k=k)
    try:
        b.run()
        check(b, qa, target, uqa, usa, ula, mode, k)
        # one unit of one query; nothing at all
        q1, uq1, us1, ul1, _ = _unit_set(rng, target, nq=1, nu=1, qlens=[100])
        _stream_and_compare(engine, b, q1, target, uq1, us1, ul1, mode, k, what="1 x 1")
        empty = np.zeros(0, dtype=np.int32)
        got, st = _stream_and_compare(engine, b, [], target, empty, empty, empty, mode, k, what="0 x 0")
        assert all(v.shape == (0,) for v in got.values()) and st["cells"] == 0 and st["scan_launches"] == 0
        # 40 queries of which the units name the even ones only
        q40, uq, us, ul, _ = _unit_set(rng, target, nq=40, nu=65)
        uq = (uq // 2) * 2
        got, _ = _stream_and_compare(engine, b, q40, target, uq, us, ul, mode, k, what="65 units, odd queries unnamed")
        assert (got["best.bestUnit"][1::2] == -1).all() and (got["best.bestUnit"][uq] >= 0).all()
        # one query named by 193 units (and by 200 below), the others by none
        q5, uq, us, ul, _ = _unit_set(rng, target, nq=5, nu=193, qlens=[60, 150, 90, 256, 1])
        uq[:] = 2
        _stream_and_compare(engine, b, q5, target, uq, us, ul, mode, k, what="193 units of one query")
        q5, uq, us, ul, _ = _unit_set(rng, target, nq=5, nu=210, qlens=[60, 150, 90, 256, 1])
        uq[:200] = 1
        _stream_and_compare(engine, b, q5, target, uq, us, ul, mode, k, what="200 units of one query")
        # every unit in the two-word group
        q2w, uq, us, ul, _ = _unit_set(rng, target, nq=20, nu=150, qlens=[33, 64] + [int(x) for x in rng.integers(33, 65, size=18)])
        _, st = _stream_and_compare(engine, b, q2w, target, uq, us, ul, mode, k, what="one word group")
        assert st["scan_launches"] == 1
        # offsets that start at 11, through the C call
        q12, uq, us, ul, _ = _unit_set(rng, target, nq=12, nu=77)
        assert _set_units_raw(b, q12, uq, us, ul, lead=11) == 0, engine.last_error()
        b.run()
        _same(_views(b), _fresh(engine, q12, target, uq, us, ul, mode, k)[0], "lead")
        check(b, q12, target, uq, us, ul, mode, k)
    finally:
        b.close()


def test_stream_the_longest_window(engine, checker):
    """a 70,000-base target and one window of exactly 65,536 columns among shorter ones"""
    target = synth.random_dna(203, 70000)
    rng = np.random.default_rng(23)
    queries, uq, us, ul, _ = _unit_set(rng, target, nq=6, nu=40, qlens=[150, 33, 256, 8, 100, 64])
    us[5], ul[5] = 4464, 65536
    us[6], ul[6] = 70000 - 65536, 65536
    b = engine.WindowBatch(queries[:2], target, [0, 1], [10, 500], [300, 200], mode="HW")
    try:
        b.run()
        _stream_and_compare(engine, b, queries, target, uq, us, ul, "HW", -1, what="65,536 columns")
    finally:
        b.close()


# ---- 3. the mapper's pattern

@pytest.mark.parametrize("start", ["empty", "pairs"])
def test_create_then_stream(engine, checker, start):
    """a batch created over no units, and one whose Create sent its only units (a 300-base query) through the internal
    pair batch: the first set_units finds the target packed and drops the pair batch"""
    target = synth.random_dna(204, 8000)
    rng = np.random.default_rng(24)
    if start == "empty":
        b = engine.WindowBatch([], target, [], [], [], mode="HW")
    else:
        b = engine.WindowBatch([_read_from(target, 1000, 300, rng, 3)], target, [0, 0], [900, 950], [500, 400], mode="HW")
    try:
        st = b.run()
        assert bool(st["path"] & 2) == (start == "pairs") and not st["path"] & 16, st
        for seed in (0, 1):
            queries, uq, us, ul, _ = _unit_set(rng, target, nq=30, nu=200)
            _, st = _stream_and_compare(engine, b, queries, target, uq, us, ul, "HW", -1, what=(start, seed))
            assert st["path"] == 16, st
    finally:
        b.close()


# ---- 4. strands

@pytest.mark.parametrize("created", ["plain", "stranded"])
def test_stream_strands(engine, checker, created):
    """a stranded set on a batch created plain, then a plain one, then an all-forward strand array; and the other way
    round"""
    target = synth.random_dna(205, 8000)
    rng = np.random.default_rng(25 + len(created))
    qa, uqa, usa, ula, sta = _unit_set(rng, target, nq=10, nu=80, strands=created == "stranded")
    b = engine.WindowBatch(qa, target, uqa, usa, ula, mode="HW", k=5, unit_strand=sta)
    try:
        b.run()
        order = ("stranded", "plain", "stranded") if created == "plain" else ("plain", "stranded", "plain")
        for i, kind in enumerate(order):
            queries, uq, us, ul, st = _unit_set(rng, target, nq=40, nu=260, strands=kind == "stranded")
            got, _ = _stream_and_compare(engine, b, queries, target, uq, us, ul, "HW", 5, st=st, what=(created, i, kind))
            if st is not None:
                ed = got["units.editDistance"]
                assert (ed[st == 1] >= 0).any() and (ed[st == 0] >= 0).any()
        queries, uq, us, ul, _ = _unit_set(rng, target, nq=12, nu=90)
        zeros = np.zeros(len(uq), dtype=np.uint8)
        b.set_units(queries, uq, us, ul, unit_strand=zeros)
        b.run()
        _same(_views(b), _fresh(engine, queries, target, uq, us, ul, "HW", 5)[0], "all forward")
    finally:
        b.close()


# ---- 5. alphabets

def _alphabet_stream(engine, target, eqs, seed, mode="HW", k=-1, spoil=None):
    rng = np.random.default_rng(seed)
    qa, uqa, usa, ula, _ = _unit_set(rng, target, nq=8, nu=50)
    b = engine.WindowBatch(qa, target, uqa, usa, ula, mode=mode, k=k, additionalEqualities=eqs)
    try:
        b.run()
        queries, uq, us, ul, _ = _unit_set(rng, target, nq=40, nu=300)
        if spoil is not None:                            # bytes the target does not hold, in every third read
            queries = [spoil(q, rng) if i % 3 == 0 and len(q) > 4 else q for i, q in enumerate(queries)]
        return _stream_and_compare(engine, b, queries, target, uq, us, ul, mode, k, eqs=eqs, what=seed)
    finally:
        b.close()


def test_stream_five_symbol_target(engine, checker):
    target = synth.masked_genome(41, 12000, frac_n=0.03, frac_lower=0.0)
    assert 5 <= len(set(target.tolist())) <= 8
    _alphabet_stream(engine, target, None, 61)


def test_stream_nine_symbol_target(engine, checker):
    target = synth.masked_genome(43, 12000, frac_n=0.03, frac_lower=0.2)
    assert 9 <= len(set(target.tolist())) <= 16
    _alphabet_stream(engine, target, None, 62, mode="SHW", k=40)


def test_stream_iupac_equalities(engine, checker):
    target = synth.masked_genome(43, 12000, frac_n=0.03, iupac=True)
    assert 9 <= len(set(target.tolist())) <= 16
    _alphabet_stream(engine, target, IUPAC, 63)


@pytest.mark.parametrize("eqs", [None, IUPAC])
def test_stream_reads_with_bytes_the_target_lacks(engine, checker, eqs):
    """N, R and a lower-case base in reads over an ACGT target: the tables are the target's, made at Create"""
    target = synth.random_dna(206, 8000)

    def spoil(q, rng):
        r = bytearray(q)
        for byte in b"NRa":
            r[int(rng.integers(0, len(r)))] = byte
        return bytes(r)
    got, _ = _alphabet_stream(engine, target, eqs, 64 + (eqs is not None), spoil=spoil)
    assert (got["units.editDistance"] >= 0).all()


# ---- 6. no stale state

def test_stream_leaves_no_stale_state(engine):
    target = synth.random_dna(207, 8000)
    rng = np.random.default_rng(27)
    a = _unit_set(rng, target, nq=40, nu=300, strands=True)
    bset = _unit_set(rng, target, nq=7, nu=33, qlens=[200, 256, 130])
    b = engine.WindowBatch(a[0], target, a[1], a[2], a[3], mode="HW", k=4, unit_strand=a[4])
    try:
        s1 = b.run()
        v1 = _views(b)
        for round_ in range(2):
            b.set_units(bset[0], bset[1], bset[2], bset[3])
            b.run()
            _views(b)
            b.set_units(a[0], a[1], a[2], a[3], unit_strand=a[4])
            s2 = b.run()
            _same(_views(b), v1, round_)
            assert {f: s1[f] for f in STATS} == {f: s2[f] for f in STATS}
    finally:
        b.close()


# ---- 7. refusals

def test_stream_refusals_leave_the_batch_as_it_was(engine):
    target = synth.random_dna(208, 70000)
    rng = np.random.default_rng(28)
    queries, uq, us, ul, _ = _unit_set(rng, target, nq=20, nu=150)
    ok = _unit_set(rng, target, nq=5, nu=9, qlens=[50, 60, 70, 80, 90])
    b = engine.WindowBatch(queries, target, uq, us, ul, mode="HW", k=6)
    try:
        b.run()
        before = _views(b)
        held = b.units(copy=False)
        held_best = b.best(copy=False)

        def unit(i, q=None, s=None, n=None, strand=None):
            """the ok set with unit i changed"""
            a = [np.array(x) for x in ok[1:4]]
            for arr, v in zip(a, (q, s, n)):
                if v is not None:
                    arr[i] = v
            st = None
            if strand is not None:
                st = np.zeros(len(a[0]), dtype=np.uint8)
                st[i] = strand
            return a + [st]

        cases = [
            ("names query 5", unit(4, q=5)), ("names query -1", unit(0, q=-1)), ("negative unitStart", unit(3, s=-1)),
            ("negative unitLength", unit(2, n=-2)), ("ends past the target", unit(7, s=69990, n=11)),
            ("unitStrand 2", unit(6, strand=2)),
        ]
        for text, (cq, cs, cl, cst) in cases:
            with pytest.raises(RuntimeError) as e:
                b.set_units(ok[0], cq, cs, cl, unit_strand=cst)
            unit_index = {"names query 5": 4, "names query -1": 0, "negative unitStart": 3, "negative unitLength": 2,
                          "ends past the target": 7, "unitStrand 2": 6}[text]
            assert text in str(e.value) and "unit %d " % unit_index in str(e.value), str(e.value)
            assert b.numQueries == len(queries) and b.numUnits == len(uq)
            _same(_views(b), before, text)
        # outside the envelope
        with pytest.raises(RuntimeError) as e:
            b.set_units(ok[0][:3] + [b"A" * 257] + ok[0][4:], ok[1], ok[2], ok[3])
        msg = str(e.value)
        assert "edlibAmdBatchWindowsSetUnits" in msg and "query 3 has 257 bases" in msg and "256" in msg, msg
        assert msg.endswith("create a new batch"), msg
        cq, cs, cl, _ = unit(8, s=100, n=65537)
        with pytest.raises(RuntimeError) as e:
            b.set_units(ok[0], cq, cs, cl)
        msg = str(e.value)
        assert "unit 8 " in msg and "65,537" in msg and "65,536" in msg and msg.endswith("create a new batch"), msg
        _same(_views(b), before, "envelope")
        # offsets, counts, pointers
        down = np.array([0, 50, 40, 180, 260, 350], dtype=np.int64)
        assert _set_units_raw(b, ok[0], ok[1], ok[2], ok[3], offsets=down) != 0
        assert "offsets" in engine.last_error() and "query 1" in engine.last_error(), engine.last_error()
        assert _set_units_raw(b, ok[0], ok[1], ok[2], ok[3], nu=-1) != 0
        assert "numUnits" in engine.last_error()
        assert _set_units_raw(b, ok[0], ok[1], ok[2], ok[3], offsets=np.zeros(0, dtype=np.int64), nu=0) != 0   # numQueries = -1
        assert "numQueries" in engine.last_error()
        L = engine.lib()
        off = np.array([0, 4], dtype=np.int64)
        one = np.zeros(1, dtype=np.int32)
        pool = np.frombuffer(b"ACGT", dtype=np.uint8)
        assert L.edlibAmdBatchWindowsSetUnits(b._h, None, None, 1, None, None, None, None, 0) != 0
        assert "NULL" in engine.last_error()
        assert L.edlibAmdBatchWindowsSetUnits(b._h, pool.ctypes.data, off.ctypes.data, 1, one.ctypes.data, None,
                                              one.ctypes.data, None, 1) != 0
        assert "NULL" in engine.last_error()
        _same(_views(b), before, "after every refusal")
        _same({"units." + f: np.array(v) for f, v in held.items()}, {f: v for f, v in before.items() if f[:5] == "units"},
              "the pinned units")
        _same({"best." + f: np.array(v) for f, v in held_best.items()}, {f: v for f, v in before.items() if f[:4] == "best"},
              "the pinned best")
        b.run()
        _same(_views(b), before, "the next run")
        # SetTargets stays refused on a window batch
        to = np.array([0, 4], dtype=np.int64)
        assert L.edlibAmdBatchCrossSetTargets(b._h, pool.ctypes.data, to.ctypes.data, 1) != 0
        assert "window batch" in engine.last_error()
        _same(_views(b), before, "SetTargets")
    finally:
        b.close()

    # a cross batch takes no units
    c = engine.CrossBatch(ok[0], [bytes(target[:300])], mode="HW")
    try:
        c.run()
        before = c.matrix()
        assert _set_units_raw(c, ok[0], ok[1], ok[2], ok[3]) != 0
        assert "edlibAmdBatchWindowsSetUnits" in engine.last_error() and "cross batch" in engine.last_error()
        assert np.array_equal(c.matrix()["editDistance"], before["editDistance"])
        c.run()
        assert np.array_equal(c.matrix()["editDistance"], before["editDistance"])
    finally:
        c.close()

    # nor does a window batch over a 17-symbol target stream any
    wide = synth.random_symbols(44, 6000, 17)
    wq = [bytes(wide[100:160]), bytes(wide[900:1000])]
    w = engine.WindowBatch(wq, wide, [0, 1, 1], [90, 880, 0], [80, 150, 100], mode="HW")
    try:
        st = w.run()
        assert st["path"] & 2 and not st["path"] & 16, st
        before = _views(w)
        with pytest.raises(RuntimeError) as e:
            w.set_units(wq, [0, 1], [90, 880], [80, 150])
        msg = str(e.value)
        assert "17 distinct symbols" in msg and "16" in msg and msg.endswith("create a new batch"), msg
        _same(_views(w), before, "17 symbols")
        w.run()
        _same(_views(w), before, "17 symbols, the next run")
    finally:
        w.close()


# ---- 8. views need a Run

def test_stream_views_need_a_run(engine):
    target = synth.random_dna(209, 8000)
    rng = np.random.default_rng(29)
    queries, uq, us, ul, _ = _unit_set(rng, target, nq=10, nu=40)
    b = engine.WindowBatch(queries, target, uq, us, ul, mode="HW")
    try:
        b.run()
        b.units()
        q2, uq2, us2, ul2, _ = _unit_set(rng, target, nq=12, nu=50)
        b.set_units(q2, uq2, us2, ul2)
        for view in (b.units, b.best):
            with pytest.raises(RuntimeError, match="Run it first"):
                view()
        v = edlib_amd.WindowView()
        assert engine.lib().edlibAmdBatchWindowView(b._h, edlib_amd.WINDOW_BEST, C.byref(v)) != 0
        b.run()
        assert b.units()["editDistance"].shape == (50,) and b.best()["bestUnit"].shape == (12,)
    finally:
        b.close()
