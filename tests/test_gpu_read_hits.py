"""-m gpu: hit-list read batches (edlibAmdBatchCreateSharedHits / edlibAmdBatchSharedHits): per read, every
maximal run of target columns that end an occurrence within k.

Every case compares all of unitOffsets / firstEnd / lastEnd / editDistance / endLocation / numLocations with
tests/hits_model.py, and ties them to a plain SharedBatch at the same k: no hit <=> editDistance -1, otherwise the least
distance over the hits is the plain one, every non-negative end location lies in a hit of that distance, and those hits'
numLocations sum to the number of non-negative end locations.  Batches that the whole-row model (hits_model.d_rows) would
take minutes for -- thousands of reads against 256,000 columns -- are modelled through seed_model.windows(), which holds
every column with D <= k and restarts the DP without changing a hit (tests/test_hits_model.py proves both on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import hits_model as H
import seed_cases as SC
import seed_model as SM
from edlib_amd import synth
from seed_cases import _mutate, _reads
from seed_model import seed_threshold

pytestmark = pytest.mark.gpu

FIELDS = ("firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]


def _nslots(n):
    return (n + 63) // 64 * 64


def _run(engine, reads, target, k, eq=None, copy=True):
    B = engine.SharedBatch(reads, target, mode="HW", task="distance", k=k, additionalEqualities=eq, hits=True)
    try:
        st = B.run()
        h = B.hits(copy=copy)
        if not copy:
            h = {f: np.array(v) if isinstance(v, np.ndarray) else v for f, v in h.items()}
        return h, st
    finally:
        B.close()


def _same(got, want):
    assert got["numHits"] == want["numHits"], (got["numHits"], want["numHits"])
    assert np.array_equal(got["unitOffsets"], want["unitOffsets"])
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, len(bad), bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def _relation2(engine, reads, target, k, eq, h):
    """the hits against a plain SharedBatch DISTANCE run at the same k"""
    B = engine.SharedBatch(reads, target, mode="HW", task="distance", k=k, additionalEqualities=eq)
    try:
        B.run()
        r = B.results_flat()
    finally:
        B.close()
    n, T = len(reads), len(target)
    off = h["unitOffsets"]
    unit = np.repeat(np.arange(n), np.diff(off))
    ed = h["editDistance"].astype(np.int64)
    best = np.full(n, 1 << 30, dtype=np.int64)
    np.minimum.at(best, unit, ed)
    nohit = np.diff(off) == 0
    assert np.array_equal(nohit, r["editDistance"] == -1)
    assert np.array_equal(best[~nohit], r["editDistance"][~nohit])
    eu = np.repeat(np.arange(n), np.diff(r["locOff"]))
    ends = r["ends"].astype(np.int64)
    keep = ends >= 0
    eu, ends = eu[keep], ends[keep]
    at = np.searchsorted(unit * (T + 1) + h["firstEnd"], eu * (T + 1) + ends, side="right") - 1
    assert (at >= 0).all()
    assert np.array_equal(unit[at], eu) and (h["lastEnd"][at] >= ends).all() and np.array_equal(ed[at], r["editDistance"][eu])
    isbest = ed == best[unit]
    total = np.zeros(n, dtype=np.int64)
    np.add.at(total, unit[isbest], h["numLocations"][isbest])
    assert np.array_equal(total, np.bincount(eu, minlength=n))
    return r


def _window_model(reads, target, k, index=None):
    """hits_csr of every read from the windows of its exact piece hits (caps off): each window restarted at its first column"""
    tb = target.tobytes()
    index = SM.build_index(tb, SM.Q) if index is None else index
    present = set(tb)
    T = len(target)
    jobs = []
    for i, r in enumerate(reads):
        assert len(r) // (k + 1) >= SM.Q
        for a, b in SM.windows(SM.lookup(r, tb, k, index=index, caps=False, present=present), len(r), k, T):
            jobs.append((i, a, b))
    n = len(reads)
    if not jobs:
        return dict({f: np.zeros(0, dtype=np.int32) for f in FIELDS}, unitOffsets=np.zeros(n + 1, dtype=np.int64), numHits=0)
    L = max(b - a + 1 for _, a, b in jobs)
    own = np.full((len(jobs), L), target[0], dtype=np.uint8)
    for j, (_, a, b) in enumerate(jobs):
        own[j, :b - a + 1] = target[a:b + 1]
    rows = H.d_rows([reads[i] for i, _, _ in jobs], own)
    c = H.hits_csr(rows, k, lengths=[b - a + 1 for _, a, b in jobs])
    per_job = np.diff(c["unitOffsets"])
    shift = np.repeat(np.array([a for _, a, _ in jobs], dtype=np.int64), per_job)
    per_read = np.bincount(np.array([i for i, _, _ in jobs]), weights=per_job, minlength=n).astype(np.int64)
    out = {"unitOffsets": np.concatenate(([0], np.cumsum(per_read))), "numHits": c["numHits"]}
    for f in FIELDS:
        out[f] = (c[f] + shift).astype(np.int32) if f in ("firstEnd", "lastEnd", "endLocation") else c[f]
    return out


# ------------------------------------------------------------------------------------ every word count, the banded path

_BANDED = {}


def _banded_case(w):
    """128 reads of 32w - 31, 32w - 16 and 32w bases against 65,536 columns: half of them planted at 1 .. 5 places with up to
    m / 4 (at most 9) edits -- among the places the target's first columns, its end, and columns 4096 and 8192 (segment
    boundaries) -- the other half unrelated; the whole rows, computed once per word count"""
    if w in _BANDED:
        return _BANDED[w]
    rng = np.random.default_rng(5000 + w)
    T = 65_536
    target = _ACGT[rng.integers(0, 4, T)].copy()
    lens = (32 * w - 31, 32 * w - 16, 32 * w)
    reads = [np.ascontiguousarray(_ACGT[rng.integers(0, 4, lens[i % 3])]) for i in range(128)]
    def plant(r, at):
        m = len(r)
        e = int(rng.integers(0, min(m // 4, 9) + 1))
        c = _mutate(rng, r, e, [int(x) for x in rng.integers(0, m, max(e, 1))]) if e else r
        at = max(0, min(at, T - len(c)))
        target[at:at + len(c)] = c
    special = lambda m: [0, T - m, 4096 - m // 2, 8192 - m + 1, 12_288 - 1, 16_384 - m // 3]
    for i in range(0, 128, 2):                                 # (planted reads alternate with unrelated ones)
        for _ in range(int(rng.integers(1, 6)) - (1 if i < 12 else 0)):
            plant(reads[i], int(rng.integers(17_000, T - 600)))          # (a later copy may cover an earlier one: the model says)
    for i in range(0, 12, 2):                                  # last, so that nothing covers them: one place each
        plant(reads[i], special(len(reads[i]))[i // 2])
    _BANDED[w] = (reads, target, H.d_rows(reads, target))
    return _BANDED[w]


@pytest.mark.parametrize("kind", ["zero", "three", "quarter"])
@pytest.mark.parametrize("w", range(1, 9))
def test_every_word_count_on_the_banded_scan(engine, w, kind):
    reads, target, rows = _banded_case(w)
    k = {"zero": 0, "three": 3, "quarter": (32 * w) // 4}[kind]
    h, st = _run(engine, reads, target, k)
    _same(h, H.hits_csr(rows, k))
    _relation2(engine, reads, target, k, None, h)
    assert st["path"] & 1
    assert st["word_steps"] >= _nslots(len(reads)) * len(target), st


# ------------------------------------------------------------------------------------------- runs across many segments

def test_runs_cut_by_every_segment_boundary(engine):
    T = 65_536 + 5
    lens = [1, 2, 31, 32, 33, 64, 100, 129, 200, 255, 256]
    target = np.full(T, ord("A"), dtype=np.uint8)
    reads = [np.full(m, ord("A"), dtype=np.uint8) for m in lens]
    for k in (0, 2, 40):
        h, st = _run(engine, reads, target, k)
        assert h["numHits"] == len(lens) and np.array_equal(h["unitOffsets"], np.arange(len(lens) + 1))
        assert np.array_equal(h["firstEnd"], [max(0, m - 1 - k) for m in lens]) and (h["lastEnd"] == T - 1).all()
        assert (h["editDistance"] == 0).all() and np.array_equal(h["endLocation"], [m - 1 for m in lens])
        assert np.array_equal(h["numLocations"], [T - m + 1 for m in lens])
        _same(h, H.hits_csr(H.d_rows(reads, target), k))
        _relation2(engine, reads, target, k, None, h)


def test_period_four_target_and_reads(engine):
    T = 65_536 - 3
    target = np.resize(_ACGT, T)
    reads = [np.resize(np.roll(_ACGT, s), m) for s, m in ((0, 4), (1, 8), (2, 33), (3, 64), (0, 130), (1, 256), (2, 1), (3, 95))]
    rows = H.d_rows(reads, target)
    for k in (0, 1, 5):
        h, _ = _run(engine, reads, target, k)
        _same(h, H.hits_csr(rows, k))
        _relation2(engine, reads, target, k, None, h)


def test_k_at_least_m_and_single_base_reads(engine):
    rng = np.random.default_rng(5100)
    T = 40_000 + 7
    target = _ACGT[rng.integers(0, 4, T)].copy()
    reads = [np.ascontiguousarray(_ACGT[rng.integers(0, 4, m)]) for m in (1, 1, 1, 1, 5, 32, 33, 150, 256)]
    reads.append(np.frombuffer(b"N", dtype=np.uint8))                       # a byte the target lacks
    rows = H.d_rows(reads, target)
    h, _ = _run(engine, reads, target, 256)                                 # k >= m: one hit [0, T - 1] per read
    assert h["numHits"] == len(reads) and (h["firstEnd"] == 0).all() and (h["lastEnd"] == T - 1).all()
    _same(h, H.hits_csr(rows, 256))
    for k in (0, 1, 5):                                                     # m = 1 at k = 0: a hit per matching column
        h, _ = _run(engine, reads, target, k)
        _same(h, H.hits_csr(rows, k))
        _relation2(engine, reads, target, k, None, h)


# --------------------------------------------------------------------------------------- wider alphabets and equalities

@pytest.mark.parametrize("eq", [False, True])
@pytest.mark.parametrize("alpha", [b"ACGTN", b"ACGTRYSWKMBDHVNX"])
def test_wider_alphabets_and_equalities(engine, alpha, eq):
    rng = np.random.default_rng(5200 + len(alpha) + eq)
    T = 20_000
    sym = np.frombuffer(alpha, dtype=np.uint8)
    p = np.full(len(alpha), 0.1 / (len(alpha) - 4))
    p[:4] = 0.9 / 4
    target = np.ascontiguousarray(rng.choice(sym, T, p=p))
    assert len(set(target.tolist())) == len(alpha)
    reads = []
    for i in range(64):
        m = int(rng.integers(1, 257))
        at = int(rng.integers(0, T - m))
        r = target[at:at + m].copy() if i % 4 else np.ascontiguousarray(rng.choice(sym, m, p=p))
        e = int(rng.integers(0, 6))
        r = _mutate(rng, r, e, [int(x) for x in rng.integers(0, m, max(e, 1))]) if e and m > 8 else r
        reads.append(np.ascontiguousarray(r[:256]))                         # (insertions must not pass the limit)
    eqs = IUPAC if eq else None
    rows = H.d_rows(reads, target, eqs)
    for k in (0, 4):
        h, st = _run(engine, reads, target, k, eqs)
        _same(h, H.hits_csr(rows, k))
        _relation2(engine, reads, target, k, eqs, h)
        assert st["word_steps"] >= _nslots(len(reads)) * T, st


# ------------------------------------------------------------------------------------------------------ the seeded path

def test_seeded_repeats_and_hand_back(engine):
    """8,192 reads against 256 kb, a 150-base block planted 20 times and another 100 times (past the bucket cap: handed back
    to the banded HITS scan), at the seed threshold"""
    rng = np.random.default_rng(811)
    T = 256_000
    target = synth.random_dna(812, T).copy()
    blocks = [synth.random_dna(813, 150), synth.random_dna(814, 150)]
    starts = rng.choice(np.arange(0, T - 150, 160), 120, replace=False)
    for j, at in enumerate(starts):
        target[at:at + 150] = blocks[0 if j < 20 else 1]
    reads = _reads(target, 8_192, 815, seed_threshold(150, T), mlo=150, mhi=150, unrelated=0.02, above=0.0, with_n=0.0)
    first = len(reads)
    for b in blocks:
        for e in range(6):
            reads.append(_mutate(rng, b, e, [int(x) for x in rng.integers(0, 150, 6)]) if e else np.ascontiguousarray(b))
    assert {(len(r) + 31) // 32 for r in reads} == {5}
    k = seed_threshold(min(len(r) for r in reads), T)
    h, st = _run(engine, reads, target, k)
    per = np.diff(h["unitOffsets"])
    assert (per[first:first + 6] == 20).all() and (per[first + 6:first + 12] == 100).all(), per[first:]
    _same(h, _window_model(reads, target, k))
    _relation2(engine, reads, target, k, None, h)
    assert st["word_steps"] < _nslots(len(reads)) * T, st


@pytest.mark.parametrize("nwd", range(1, 9))
def test_seed_pass_is_the_only_scan(engine, nwd):
    """a planted batch per word count at its seed threshold, nothing handed back: word_steps == NWD x the columns of the
    model's merged windows, each window counted once"""
    b = SC.single_group(nwd, seed_threshold(SC.M_MIN[nwd], 256_000), mlo=SC.M_MIN[nwd])
    k, reads, target = b["k"], b["reads"], b["target"]
    assert 0 <= k <= seed_threshold(min(len(r) for r in reads), len(target))
    assert 1_024 <= _nslots(len(reads)) < 16_384 and _nslots(len(reads)) * len(target) >= 1 << 30
    index = SM.build_index(target.tobytes(), SM.Q)
    pred = [SM.predict(r, target.tobytes(), k, index, set(target.tobytes())) for r in reads]
    assert sum(p["back"] for p in pred) == 0
    h, st = _run(engine, reads, target, k)
    _same(h, _window_model(reads, target, k, index))
    _relation2(engine, reads, target, k, None, h)
    assert st["word_steps"] == nwd * sum(p["columns"] for p in pred), st


def test_five_symbol_target_keeps_the_banded_scan(engine):
    b = SC.five_symbols()
    reads, target, k = b["reads"], b["target"], 8
    assert len(set(target.tolist())) == 5
    h, st = _run(engine, reads, target, k)
    _same(h, _window_model(reads, target, k))
    _relation2(engine, reads, target, k, None, h)
    assert st["word_steps"] >= _nslots(len(reads)) * len(target), st


# --------------------------------------------------------------------------------------------------------- list growth

_GROWTH = []


def _growth_case():
    """a 24-mer planted 300 times in 65,536 columns and its hits at k = 1: 4,096 copies of it pass the list's first 2^20 entries"""
    if not _GROWTH:
        rng = np.random.default_rng(5300)
        T = 65_536
        target = _ACGT[rng.integers(0, 4, T)].copy()
        mer = np.ascontiguousarray(_ACGT[rng.integers(0, 4, 24)])
        for at in 100 + 200 * np.arange(300):                               # 300 copies, 200 columns apart
            target[at:at + 24] = mer
        one = H.hits_csr(H.d_rows([mer], target), 1)
        assert one["numHits"] >= 300 and 4_096 * one["numHits"] > 1 << 20
        _GROWTH.append((target, mer, one))
    return _GROWTH[0]


def test_list_grows_once_and_later_runs_fit(engine):
    target, mer, one = _growth_case()
    n = 4_096
    want = {f: np.tile(one[f], n) for f in FIELDS}
    want["unitOffsets"] = np.arange(n + 1, dtype=np.int64) * one["numHits"]
    want["numHits"] = n * one["numHits"]
    B = engine.SharedBatch([mer] * n, target, mode="HW", task="distance", k=1, hits=True)
    try:
        st1 = B.run()
        _same(B.hits(), want)
        st2 = B.run()
        _same(B.hits(), want)
    finally:
        B.close()
    assert st2["scan_launches"] < st1["scan_launches"], (st1, st2)


def test_empty_reads_behind_a_list_that_grows(engine):
    """the batch above with an empty read first, in the middle and last: the rows answered on the host go in behind the scans'
    runs, here into a list that has just grown to hold both"""
    target, mer, one = _growth_case()
    T, n = len(target), 4_096
    empty = H.hits_csr(H.d_row(b"", target)[None, :], 1)                    # (row -1 of the recurrence: zeros)
    assert empty["numHits"] == 1 and tuple(int(empty[f][0]) for f in FIELDS) == (0, T - 1, 0, 0, T)
    reads = [b""] + [mer] * (n // 2) + [b""] + [mer] * (n // 2) + [b""]
    per = [empty if len(r) == 0 else one for r in reads]
    want = {f: np.concatenate([c[f] for c in per]) for f in FIELDS}
    want["unitOffsets"] = np.concatenate(([0], np.cumsum([c["numHits"] for c in per]))).astype(np.int64)
    want["numHits"] = int(want["unitOffsets"][-1])
    assert n * one["numHits"] <= 1 << 30
    B = engine.SharedBatch(reads, target, mode="HW", task="distance", k=1, hits=True)
    try:
        st1 = B.run()
        h1 = B.hits()
        st2 = B.run()
        h2 = B.hits()
    finally:
        B.close()
    for h in (h1, h2):
        _same(h, want)
        off = h["unitOffsets"]
        for u in (0, n // 2 + 1, n + 2):
            assert off[u + 1] - off[u] == 1
            assert tuple(int(h[f][off[u]]) for f in FIELDS) == (0, T - 1, 0, 0, T), u
    assert st2["scan_launches"] < st1["scan_launches"], (st1, st2)


# ------------------------------------------------------------------------------------------------ refusals and empties

def _create(engine, reads, target, mode="HW", task="distance", k=2):
    L = engine.lib()
    cfg, _ = engine._make_config(mode, task, k, None)
    qd, qo = engine._pack(list(reads))
    t = np.frombuffer(bytes(target), dtype=np.uint8)
    h = L.edlibAmdBatchCreateSharedHits(qd.ctypes.data, qo.ctypes.data, len(reads), t.ctypes.data, len(target), cfg, 0)
    return h, engine.last_error()


def test_refusals_name_the_limit(engine):
    ok = ([b"ACGTACGT"], b"ACGTACGTAC")
    for kw, names in ((dict(k=-1), "k must be >= 0"), (dict(mode="SHW"), "EDLIB_MODE_HW"), (dict(mode="NW"), "EDLIB_MODE_HW"),
                      (dict(task="locations"), "EDLIB_TASK_DISTANCE"), (dict(task="path"), "EDLIB_TASK_DISTANCE")):
        h, err = _create(engine, *ok, **kw)
        assert not h and names in err, (kw, err)
    h, err = _create(engine, [b"ACGT", b"A" * 257], ok[1])
    assert not h and "the limit is 256" in err, err
    h, err = _create(engine, ok[0], bytes(range(65, 82)))
    assert not h and "the limit is 16" in err, err


def test_other_views_fail_on_a_hits_batch_and_hits_on_a_plain_one(engine):
    L = engine.lib()
    h, err = _create(engine, [b"ACGTACGT"], b"TTACGTACGTTT")
    assert h, err
    try:
        v = engine.ReadHits()
        assert L.edlibAmdBatchSharedHits(h, C.byref(v)) != 0 and "Run it first" in engine.last_error()
        assert L.edlibAmdBatchRun(h) == 0
        res = (engine.AlignResult * 1)()
        assert L.edlibAmdBatchResults(h, res) != 0 and "hit-list" in engine.last_error()
        rv = engine.ResultsView()
        assert L.edlibAmdBatchResultsView(h, C.byref(rv)) != 0 and "hit-list" in engine.last_error()
        assert L.edlibAmdBatchResultsFlat(h, *([None] * 9)) != 0
        pc, po = C.c_void_p(), C.c_void_p()
        assert L.edlibAmdBatchCigarView(h, 1, C.byref(pc), C.byref(po)) != 0
        sv = engine.StrandView()
        assert L.edlibAmdBatchStrandView(h, C.byref(sv)) != 0
        cv = engine.CrossView()
        assert L.edlibAmdBatchCrossView(h, engine.CROSS_BEST, C.byref(cv)) != 0
        ch = engine.CrossHits()
        assert L.edlibAmdBatchCrossHits(h, C.byref(ch)) != 0
        assert L.edlibAmdBatchSharedHits(h, C.byref(v)) == 0 and v.numHits == 1
    finally:
        L.edlibAmdBatchDestroy(h)
    plain = engine.SharedBatch([b"ACGTACGT"], b"TTACGTACGTTT", k=2)
    try:
        plain.run()
        v = engine.ReadHits()
        assert L.edlibAmdBatchSharedHits(plain._h, C.byref(v)) != 0 and "not a hit-list read batch" in engine.last_error()
        with pytest.raises(RuntimeError, match="hits=True"):
            plain.hits()
    finally:
        plain.close()
    cross = engine.CrossBatch([b"ACGT"], [b"ACGTAC"], k=1, hits=True)
    try:
        cross.run()
        assert L.edlibAmdBatchSharedHits(cross._h, C.byref(v)) != 0
    finally:
        cross.close()


def test_empty_reads_empty_target_and_empty_batch(engine):
    target = np.frombuffer(b"TTACGTACGTTTACGAACGT", dtype=np.uint8)
    T = len(target)
    reads = [b"", b"ACGTACGT", b"", b"GGGGGGGG", b"ACG"]
    for copy in (True, False):
        h, st = _run(engine, reads, target, 1, copy=copy)
        rows = H.d_rows([r for r in reads if r], target)
        want = H.hits_csr(rows, 1)
        per = iter(np.diff(want["unitOffsets"]))
        counts = [1 if not r else next(per) for r in reads]                 # an empty read hits once
        assert np.array_equal(np.diff(h["unitOffsets"]), counts)
        off = h["unitOffsets"]
        for u in (0, 2):
            got = tuple(int(h[f][off[u]]) for f in FIELDS)
            assert got == (0, T - 1, 0, 0, T), got
        keep = np.ones(h["numHits"], dtype=bool)
        keep[[off[0], off[2]]] = False
        for f in FIELDS:
            assert np.array_equal(h[f][keep], want[f]), f
        assert st["path"] & 1
    h, _ = _run(engine, reads, b"", 1)                                      # T == 0: no read has a hit
    assert h["numHits"] == 0 and np.array_equal(h["unitOffsets"], np.zeros(len(reads) + 1))
    h, _ = _run(engine, [b"", b""], target, 0)                              # only empty reads: nothing is scanned
    assert h["numHits"] == 2 and np.array_equal(h["lastEnd"], [T - 1, T - 1]) and np.array_equal(h["numLocations"], [T, T])
    h, _ = _run(engine, [], target, 1)                                      # numQueries = 0
    assert h["numHits"] == 0 and np.array_equal(h["unitOffsets"], [0])
    h, _ = _run(engine, [b"GGGGGGGG"], target, 0, copy=False)               # nothing within k
    assert h["numHits"] == 0 and np.array_equal(h["unitOffsets"], [0, 0])
    assert engine.find_all([b"ACGTACGT"], target, 0)["endLocation"].tolist() == [9]


# ----------------------------------------------------------------------------------------------------------- read order

def test_unit_offsets_follow_the_callers_order(engine):
    """all eight word counts in shuffled order: the groups permute the slots, unitOffsets must not"""
    rng = np.random.default_rng(5400)
    T = 30_000
    target = _ACGT[rng.integers(0, 4, T)].copy()
    reads = []
    for i in range(200):
        m = int(rng.integers(32 * (i % 8) + 1, 32 * (i % 8) + 33))
        at = int(rng.integers(0, T - m))
        e = int(rng.integers(0, 4))
        r = target[at:at + m].copy()
        r = _mutate(rng, r, e, [int(x) for x in rng.integers(0, m, max(e, 1))]) if e and m > 8 else r
        reads += SC.fit_lengths([r], 32 * (i % 8) + 1, 32 * (i % 8) + 32, 5401 + i)   # (indels must not move it to another word count)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    assert {(len(r) + 31) // 32 for r in reads} == set(range(1, 9))
    h, _ = _run(engine, reads, target, 3)
    _same(h, H.hits_csr(H.d_rows(reads, target), 3))
    _relation2(engine, reads, target, 3, None, h)


# --------------------------------------------------------------------------------------------------------------- C ABI

def test_c_abi_and_the_callers_device(engine):
    """the two functions driven from C through ctypes without the Python class; Create / Run / SharedHits on a chosen device
    leave the calling thread's current device where it was"""
    hip = C.CDLL("libamdhip64.so")

    def current():
        d = C.c_int(-1)
        assert hip.hipGetDevice(C.byref(d)) == 0
        return d.value
    assert hip.hipSetDevice(0) == 0
    L = engine.lib()
    reads = [b"ACGTACGT", b"TTTT", b"GATTACA"]
    target = b"TTACGTACGTTTTTGATTACATT"
    pool = b"".join(reads)
    offs = (C.c_longlong * 4)(0, 8, 12, 19)
    cfg = L.edlibNewAlignConfig(1, 2, 0, None, 0)
    dev = engine.device_count() - 1
    h = L.edlibAmdBatchCreateSharedHits(pool, offs, 3, target, len(target), cfg, dev)
    assert h, engine.last_error()
    try:
        assert current() == 0
        assert L.edlibAmdBatchRun(h) == 0, engine.last_error()
        assert current() == 0
        v = engine.ReadHits()
        assert L.edlibAmdBatchSharedHits(h, C.byref(v)) == 0, engine.last_error()
        assert current() == 0
        assert v.numUnits == 3
        rows = H.d_rows(reads, target)
        want = H.hits_csr(rows, 1)
        assert v.numHits == want["numHits"]
        assert [v.unitOffsets[i] for i in range(4)] == want["unitOffsets"].tolist()
        for f in FIELDS:
            assert [getattr(v, f)[i] for i in range(v.numHits)] == want[f].tolist(), f
        st = engine.BatchStats()
        assert L.edlibAmdBatchStats(h, C.byref(st)) == 0 and st.path & 1 and st.word_steps > 0
    finally:
        L.edlibAmdBatchDestroy(h)
    assert current() == 0
