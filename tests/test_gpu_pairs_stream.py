"""GPU: streamed pairs (edlibAmdBatchPairsSetPairs, PairBatch.set_pairs): a resident pair batch whose pairs are replaced
must be, after its next run(), exactly a fresh PairBatch created over the same pairs -- every array of results_flat(),
both CIGAR forms and the statistics that describe the work -- and a strided sample (or all) of its units must equal the
checker; a refused set must leave the batch as it was."""
import ctypes as C

import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth
from pairs_set_cases import IUPAC, STATS, check as _check, fresh as _fresh, same as _same, snapshot as _snapshot

pytestmark = pytest.mark.gpu

ACGT = b"ACGT"
AMINO = b"ACDEFGHIKLMNPQRSTVWY"


def _pair(rng, m, mode, alphabet=ACGT, qalphabet=None, sub=0.03, T=None):
    """one (query of m bases, target) pair: NW a target of about m bases, SHW / HW a target the query was cut from; a few
    substitutions (from qalphabet: bytes the target may not hold) and now and then an indel"""
    A = np.frombuffer(alphabet, dtype=np.uint8)
    Q = A if qalphabet is None else np.frombuffer(qalphabet, dtype=np.uint8)
    if T is None:
        T = max(1, m + int(rng.integers(-(m // 10), m // 10 + 1))) if mode == "NW" else m + int(rng.integers(0, 2 * m + 40))
    t = A[rng.integers(0, len(A), size=T)]
    s = 0 if mode != "HW" else int(rng.integers(0, max(T - m, 0) + 1))
    q = t[s:s + m].copy()
    if len(q) < m:
        q = np.concatenate([q, Q[rng.integers(0, len(Q), size=m - len(q))]])
    at = rng.integers(0, m, size=rng.binomial(m, sub))
    q[at] = Q[rng.integers(0, len(Q), size=len(at))]
    if m > 4 and rng.random() < 0.3:
        p = int(rng.integers(1, m - 1))
        q = np.concatenate([q[:p], q[p + 1:], Q[rng.integers(0, len(Q), size=1)]])
    return q.tobytes(), t.tobytes()


def _pairs(rng, n, mode, lo=30, hi=300, **kw):
    out = [_pair(rng, int(m), mode, **kw) for m in rng.integers(lo, hi + 1, size=n)]
    return [q for q, _ in out], [t for _, t in out]


def _stream_and_compare(engine, checker, b, qs, ts, mode, task, k, eqs=None, everything=False, stats_equal=True, what=""):
    """set_pairs + run on b against a fresh batch over the same pairs, and about 100 units (or all) against the checker"""
    b.set_pairs(qs, ts)
    assert b.n == len(qs)
    stats = b.run()
    got = _snapshot(b)
    want, wstats = _fresh(engine, qs, ts, mode, task, k, eqs)
    _same(got, want, what)
    if stats_equal:
        assert {f: stats[f] for f in STATS} == {f: wstats[f] for f in STATS}, what
    assert stats["cells"] == sum(len(q) * len(t) for q, t in zip(qs, ts)), what
    n = len(qs)
    _check(b, checker, qs, ts, mode, task, k, eqs, None if everything else range(0, n, max(1, n // 100)), what)
    return got, stats


# ---- 1. stream equals a fresh batch

@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("task", ["distance", "locations", "path"])
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_stream_equals_fresh_batch(engine, checker, mode, task, k):
    rng = np.random.default_rng(["NW", "SHW", "HW"].index(mode) * 100 + ["distance", "locations", "path"].index(task) * 10 + k + 1)
    qa, ta = _pairs(rng, 1200, mode, 50, 120)
    # (SHW / HW paths: a streamed set takes queries up to 256 bases -- the flat envelope; 257 is refused below)
    longest = 256 if task == "path" and mode != "NW" else 300
    b = engine.PairBatch(qa, ta, mode=mode, task=task, k=k)
    try:
        b.run()
        _snapshot(b)
        for c, (n, lo, hi) in enumerate(((1900, 30, longest), (1100, 30, 90), (1500, 100, 250))):
            qs, ts = _pairs(rng, n, mode, lo, hi)
            got, stats = _stream_and_compare(engine, checker, b, qs, ts, mode, task, k, what=(mode, task, k, c))
            assert stats["path"] & 2 and (got["editDistance"] >= 0).any()
            if k >= 0:
                assert (got["editDistance"] == -1).any()
    finally:
        b.close()


# ---- 2. counts: no count below 1,024 ever ran flat before, so every unit goes to the checker

@pytest.mark.parametrize("mode,task", [("HW", "path"), ("NW", "path"), ("SHW", "locations"), ("HW", "distance")])
def test_counts_big_small_big(engine, checker, mode, task):
    rng = np.random.default_rng(77 + len(mode) + len(task))
    b = engine.PairBatch([], [], mode=mode, task=task)
    try:
        for n in (1500, 0, 1023, 1, 1500, 63, 64, 65, 1500):
            qs, ts = _pairs(rng, n, mode, 30, 200)
            # (a fresh batch of fewer than 1,024 pairs takes the general path: its word_steps and launches are another count)
            got, stats = _stream_and_compare(engine, checker, b, qs, ts, mode, task, -1, everything=True,
                                             stats_equal=n >= 1024, what=(mode, task, n))
            assert len(got["editDistance"]) == n and stats["path"] == (2 if n else 0), (n, stats)
    finally:
        b.close()


# ---- 3. ring and block edges across chunks

@pytest.mark.parametrize("mode,task", [("NW", "distance"), ("HW", "locations"), ("SHW", "distance"), ("NW", "path")])
def test_longest_query_moves_the_ring(engine, checker, mode, task):
    rng = np.random.default_rng(31 + len(mode) + len(task))
    b = engine.PairBatch([], [], mode=mode, task=task)
    try:
        for longest in (256, 257, 512, 513, 1024, 100):
            qs, ts = _pairs(rng, 1100, mode, 30, 100)
            for at, m in ((0, longest), (577, longest), (1099, max(longest - 1, 1))):
                qs[at], ts[at] = _pair(rng, m, mode)
            got, _ = _stream_and_compare(engine, checker, b, qs, ts, mode, task, -1, what=(mode, task, longest))
            _check(b, checker, qs, ts, mode, task, -1, sel=(0, 577, 1099), what=("long", longest))
    finally:
        b.close()


def test_nw_paths_of_1kb_then_100bp(engine, checker):
    """rings of 32-row words: queries above 8 words take band level 128 (similar pairs stay inside it)"""
    rng = np.random.default_rng(5)
    b = engine.PairBatch([], [], mode="NW", task="path")
    try:
        qs, ts = _pairs(rng, 1100, "NW", 900, 1024, sub=0.02)
        _stream_and_compare(engine, checker, b, qs, ts, "NW", "path", -1, what="1 kb")
        qs, ts = _pairs(rng, 1300, "NW", 60, 140)
        _stream_and_compare(engine, checker, b, qs, ts, "NW", "path", -1, what="100 bp")
    finally:
        b.close()


@pytest.mark.parametrize("task", ["distance", "path"])
def test_a_target_of_65536_bases(engine, checker, task):
    rng = np.random.default_rng(6)
    b = engine.PairBatch([], [], mode="HW", task=task)
    try:
        qs, ts = _pairs(rng, 1100, "HW", 30, 120)
        qs[500], ts[500] = _pair(rng, 100, "HW", T=65536)
        _stream_and_compare(engine, checker, b, qs, ts, "HW", task, -1, what="65536")
        _check(b, checker, qs, ts, "HW", task, -1, sel=(500,), what="65536")
    finally:
        b.close()


# ---- 4. alphabets on one batch

@pytest.mark.parametrize("mode,task", [("HW", "path"), ("NW", "path"), ("SHW", "distance")])
def test_alphabets_on_one_batch(engine, checker, mode, task):
    rng = np.random.default_rng(41 + len(mode))
    b = engine.PairBatch([], [], mode=mode, task=task)
    try:
        for alphabet in (ACGT, b"ACGTN", AMINO, ACGT):
            qs, ts = _pairs(rng, 1200, mode, 30, 200, alphabet=alphabet)
            got, _ = _stream_and_compare(engine, checker, b, qs, ts, mode, task, -1, what=(mode, task, alphabet))
            assert got["alphabetLength"].max() == len(alphabet)
        # queries with bytes no target has: they are counted in alphabetLength and match nothing
        qs, ts = _pairs(rng, 1200, mode, 30, 200, alphabet=ACGT, qalphabet=b"ACGTNRYxz", sub=0.1)
        got, _ = _stream_and_compare(engine, checker, b, qs, ts, mode, task, -1, what="foreign query bytes")
        assert got["alphabetLength"].max() > 4
    finally:
        b.close()


@pytest.mark.parametrize("mode,task", [("HW", "locations"), ("NW", "path")])
def test_iupac_equalities_stay_with_the_batch(engine, checker, mode, task):
    rng = np.random.default_rng(43)
    b = engine.PairBatch([], [], mode=mode, task=task, additionalEqualities=IUPAC)
    try:
        for alphabet, qalphabet in ((b"ACGT", b"ACGTRYN"), (b"ACGTN", b"ACGTRY"), (b"ACGTRYN", b"ACGT")):
            qs, ts = _pairs(rng, 1150, mode, 30, 200, alphabet=alphabet, qalphabet=qalphabet, sub=0.08)
            _stream_and_compare(engine, checker, b, qs, ts, mode, task, -1, eqs=IUPAC, what=(mode, alphabet))
    finally:
        b.close()


# ---- 5. fall-backs of a Run after a stream: whatever the general path reads must describe the new set

@pytest.mark.parametrize("task", ["distance", "locations", "path"])
def test_more_than_16_end_locations_after_a_stream(engine, checker, task):
    rng = np.random.default_rng(51)
    b = engine.PairBatch([], [], mode="HW", task=task)
    try:
        qs, ts = _pairs(rng, 1700, "HW", 30, 200)
        _stream_and_compare(engine, checker, b, qs, ts, "HW", task, -1, what="before")
        qs, ts = _pairs(rng, 1200, "HW", 30, 200)
        for at in (3, 700, 1199):
            qs[at], ts[at] = b"A" * 40, b"A" * 200            # 161 end locations at distance 0
        got, stats = _stream_and_compare(engine, checker, b, qs, ts, "HW", task, -1, what=("overflow", task))
        assert got["numLocations"][3] == 161
        assert stats["overflow_units"] == 3 if task == "distance" else True
        _check(b, checker, qs, ts, "HW", task, -1, sel=(3, 700, 1199), what=("overflow", task))
    finally:
        b.close()


def test_failed_band_level_after_a_stream(engine, checker):
    rng = np.random.default_rng(52)
    b = engine.PairBatch([], [], mode="NW", task="path")
    try:
        qs, ts = _pairs(rng, 1600, "NW", 30, 200)
        _stream_and_compare(engine, checker, b, qs, ts, "NW", "path", -1, what="before")
        qs, ts = _pairs(rng, 1150, "NW", 30, 200)
        # more than 8 words and unrelated: the distance is far above the first level's 128
        qs[9] = synth.random_dna(1, 400).tobytes()
        ts[9] = synth.random_dna(2, 400).tobytes()
        got, _ = _stream_and_compare(engine, checker, b, qs, ts, "NW", "path", -1, what="failed level")
        assert got["editDistance"][9] > 128
        _check(b, checker, qs, ts, "NW", "path", -1, sel=(9,), what="failed level")
    finally:
        b.close()


# ---- 6. no stale views

def test_no_stale_views(engine, checker):
    rng = np.random.default_rng(61)
    qa, ta = _pairs(rng, 1300, "HW", 30, 200)
    qb, tb = _pairs(rng, 1250, "HW", 30, 200)
    b = engine.PairBatch(qa, ta, mode="HW", task="path")
    try:
        b.run()
        b.results_flat()
        b.cigars()
        b.set_pairs(qb, tb)
        for view in (b.results_flat, b.cigars, b.results):
            with pytest.raises(RuntimeError, match="Run it first"):
                view()
        b.run()
        first = _snapshot(b)
        want, _ = _fresh(engine, qb, tb, "HW", "path", -1)
        _same(first, want, "after the set")
        b.set_pairs(qb, tb)
        b.run()
        _same(_snapshot(b), first, "the same set again")
        b.run()
        _same(_snapshot(b), first, "a second run")
    finally:
        b.close()


# ---- 7. create, then stream

@pytest.mark.parametrize("made_over", ["nothing", "40 pairs", "a 5 kb pair", "an empty target"])
def test_create_then_stream(engine, checker, made_over):
    rng = np.random.default_rng(71)
    qa, ta = {"nothing": lambda: ([], []), "40 pairs": lambda: _pairs(rng, 40, "HW"),
              "a 5 kb pair": lambda: _pairs(rng, 1100, "HW", 30, 100),
              "an empty target": lambda: _pairs(rng, 1100, "HW", 30, 100)}[made_over]()
    if made_over == "a 5 kb pair":
        qa[7], ta[7] = _pair(rng, 5000, "HW")
    if made_over == "an empty target":
        ta[7] = b""
    b = engine.PairBatch(qa, ta, mode="HW", task="locations")
    try:
        b.run()
        if qa:
            _check(b, checker, qa, ta, "HW", "locations", -1, sel=range(0, len(qa), 50), what=made_over)
        qs, ts = _pairs(rng, 1400, "HW", 30, 250)
        _stream_and_compare(engine, checker, b, qs, ts, "HW", "locations", -1, what=made_over)
    finally:
        b.close()


# ---- 8. refusals leave the batch as it was

def _pack(seqs, lead=0):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"x" * lead + b"".join(seqs) + b"\0", dtype=np.uint8), off + lead


def _set_pairs_raw(b, qs, ts, lead=0, qoff=None, toff=None, n=None):
    """edlibAmdBatchPairsSetPairs on the handle itself: `lead` bytes in front of the pools, offsets of the caller's own"""
    qp, qo = _pack(qs, lead)
    tp, to = _pack(ts, lead)
    qo = qo if qoff is None else np.asarray(qoff, dtype=np.int64)
    to = to if toff is None else np.asarray(toff, dtype=np.int64)
    return edlib_amd.lib().edlibAmdBatchPairsSetPairs(b._h, qp.ctypes.data, qo.ctypes.data, tp.ctypes.data, to.ctypes.data,
                                                      len(qs) if n is None else n)


def test_offsets_need_not_start_at_zero(engine, checker):
    rng = np.random.default_rng(80)
    qs, ts = _pairs(rng, 1100, "NW", 30, 150)
    b = engine.PairBatch([], [], mode="NW", task="path")
    try:
        assert _set_pairs_raw(b, qs, ts, lead=37) == 0, engine.last_error()
        b.n = len(qs)
        b.run()
        want, _ = _fresh(engine, qs, ts, "NW", "path", -1)
        _same(_snapshot(b), want, "lead 37")
    finally:
        b.close()


@pytest.mark.parametrize("mode,task", [("HW", "path"), ("NW", "path"), ("SHW", "path")])
def test_refusals_leave_the_batch_as_it_was(engine, checker, mode, task):
    rng = np.random.default_rng(81 + len(mode))
    qa, ta = _pairs(rng, 1200, mode, 30, 200)
    qs, ts = _pairs(rng, 1100, mode, 30, 100)
    b = engine.PairBatch(qa, ta, mode=mode, task=task)
    try:
        b.run()
        before = _snapshot(b)

        def refused(call, *words):
            held = b.results_flat(copy=False)                  # views of the batch's own memory, held across the refusal
            cig = b.cigars(copy=False)
            assert call() != 0
            msg = engine.last_error()
            assert "edlibAmdBatchPairsSetPairs" in msg and all(w in msg for w in words), msg
            assert b.n == len(qa)
            for f, v in held.items():
                assert v is None or np.array_equal(v, before[f]), (msg, f)
            assert np.array_equal(cig[0], before["cigar1.chars"]) and np.array_equal(cig[1], before["cigar1.off"]), msg
            _same(_snapshot(b), before, msg)
            del held, cig
            b.run()                                            # ... and the next Run reproduces them
            _same(_snapshot(b), before, ("the next run", msg))

        def with_pair(at, q, t):
            q2, t2 = list(qs), list(ts)
            q2[at], t2[at] = q, t
            return lambda: _set_pairs_raw(b, q2, t2)

        L = engine.lib()
        one = np.zeros(2, dtype=np.int64)
        refused(lambda: L.edlibAmdBatchPairsSetPairs(b._h, None, None, None, None, 1), "NULL")
        refused(lambda: L.edlibAmdBatchPairsSetPairs(b._h, one.ctypes.data, one.ctypes.data, None, one.ctypes.data, 1), "NULL")
        refused(lambda: _set_pairs_raw(b, qs, ts, n=-1), "numPairs", "-1")
        down = _pack(qs)[1].copy()
        down[6] = down[5] - 1
        refused(lambda: _set_pairs_raw(b, qs, ts, qoff=down), "bad query offsets", "query 5")
        down = _pack(ts)[1].copy()
        down[11] = down[10] - 3
        refused(lambda: _set_pairs_raw(b, qs, ts, toff=down), "bad target offsets", "target 10")
        refused(with_pair(17, b"", ts[17]), "pair 17", "empty query", "create a new batch")
        refused(with_pair(1099, qs[1099], b""), "pair 1099", "empty target", "create a new batch")
        refused(with_pair(4, b"A" * 1025, b"A" * 1000), "pair 4", "1,025", "1,024", "create a new batch")
        refused(with_pair(0, qs[0], b"C" * 65537), "pair 0", "65,537", "65,536", "create a new batch")
        if mode != "NW":
            refused(with_pair(600, b"G" * 257, b"G" * 300), "pair 600", "257", "256", "EDLIB_TASK_PATH", "create a new batch")
        # the linear-space regime: (20 blocks + 8) T >= 1 MiB
        m, T = (1000, 3200) if mode == "NW" else (256, 12000)
        hirschberg = with_pair(33, b"A" * m, b"A" * T)
        if mode == "HW" or mode == "SHW":
            # (SHW / HW look at the window of 2 m + 1 columns: 513 x 4 blocks stay below the rule -- such a pair is taken)
            assert hirschberg() == 0, engine.last_error()
            b.set_pairs(qa, ta)
            b.run()
            _same(_snapshot(b), before, "the first set again")
        else:
            refused(hirschberg, "pair 33", "1,000", "3,200", "linear-space", "create a new batch")
        b.run()                                                # the next Run reproduces the views
        _same(_snapshot(b), before, "the next run")
        # ... and a set that is taken still goes through
        _stream_and_compare(engine, checker, b, qs, ts, mode, task, -1, what="after the refusals")
    finally:
        b.close()


def test_other_kinds_of_batch_are_refused_by_name(engine):
    reads = [b"ACGTACGTAC", b"TTGACCA"]
    target = synth.random_dna(9, 400).tobytes()
    z = np.zeros(1, dtype=np.int32)
    kinds = [
        (lambda: engine.SharedBatch(reads, target), "a shared-target read batch"),
        (lambda: engine.BothStrandsBatch(reads, target), "a both-strand read batch"),
        (lambda: engine.SharedBatch(reads, target, k=2, hits=True), "a hit-list read batch"),
        (lambda: engine.CrossBatch(reads, [target]), "a cross batch"),
        (lambda: engine.SelfBatch(reads), "a self batch"),
        (lambda: engine.CrossBatch(reads, [target], k=2, occurrences=True), "an occurrence batch"),
        (lambda: engine.WindowBatch(reads, target, z, z, z + 50), "a window batch"),
    ]
    qp, qo = _pack(reads)
    for make, kind in kinds:
        b = make()
        try:
            b.run()
            assert engine.lib().edlibAmdBatchPairsSetPairs(b._h, qp.ctypes.data, qo.ctypes.data, qp.ctypes.data,
                                                           qo.ctypes.data, 2) != 0
            msg = engine.last_error()
            assert "edlibAmdBatchPairsSetPairs" in msg and kind in msg, msg
            b.run()                                            # the batch is what it was
        finally:
            b.close()
    # a pair batch of ONE pair is a shared-target batch inside: it is still a pair batch
    b = engine.PairBatch([reads[0]], [target], mode="HW", task="locations")
    try:
        b.run()
        b.set_pairs(reads, [target, target])
        b.run()
        assert len(b.results_flat()["editDistance"]) == 2
    finally:
        b.close()


# ---- 9. Create: what shares the builder with the stream

def test_create_pairs_over_null_pointers(engine):
    """a resident batch made over nothing at all (the C form of PairBatch([], [])) takes a chunk"""
    L = engine.lib()
    cfg, keep = edlib_amd._make_config("HW", "locations", -1, None)
    h = L.edlibAmdBatchCreatePairs(None, None, None, None, 0, cfg, 0)
    assert h, engine.last_error()
    try:
        assert L.edlibAmdBatchRun(h) == 0, engine.last_error()
        rng = np.random.default_rng(91)
        qs, ts = _pairs(rng, 1100, "HW", 30, 100)
        qp, qo = _pack(qs)
        tp, to = _pack(ts)
        assert L.edlibAmdBatchPairsSetPairs(h, qp.ctypes.data, qo.ctypes.data, tp.ctypes.data, to.ctypes.data, len(qs)) == 0, engine.last_error()
        assert L.edlibAmdBatchRun(h) == 0, engine.last_error()
        ed = np.zeros(len(qs), dtype=np.int32)
        assert L.edlibAmdBatchResultsFlat(h, None, ed.ctypes.data, None, None, None, None, None, None, None) == 0, engine.last_error()
        want, _ = _fresh(engine, qs, ts, "HW", "locations", -1)
        assert np.array_equal(ed, want["editDistance"])
    finally:
        L.edlibAmdBatchDestroy(h)


@pytest.mark.parametrize("mode,task", [("NW", "distance"), ("SHW", "locations"), ("HW", "path"), ("NW", "path"), ("HW", "distance")])
def test_shared_target_batch_of_pair_units_stays_flat(engine, checker, mode, task):
    """Create's flat path also serves a shared-target batch whose reads are all pair units (a target of more symbols than
    the reads-per-lane kernels take: protein): every unit's target is the one target, and every unit equals the checker"""
    rng = np.random.default_rng(95 + len(mode) + len(task))
    A = np.frombuffer(AMINO, dtype=np.uint8)
    target = A[rng.integers(0, 20, size=700)].tobytes()
    reads = []
    for m in rng.integers(20, 257, size=1100):
        s = int(rng.integers(0, len(target) - int(m) + 1))
        q = np.frombuffer(target[s:s + int(m)], dtype=np.uint8).copy()
        at = rng.integers(0, m, size=rng.binomial(m, 0.05))
        q[at] = A[rng.integers(0, 20, size=len(at))]
        reads.append(q.tobytes())
    if mode == "HW":
        reads[5] = target[100:101] * 60                        # one residue repeated: ties -- where they pass 16 end locations, the exact second pass / the general path
    b = engine.SharedBatch(reads, target, mode=mode, task=task)
    try:
        stats = b.run()
        assert stats["path"] == 2 and stats["cells"] == sum(len(q) for q in reads) * len(target), stats
        f = b.results_flat()
        assert len(f["editDistance"]) == len(reads) and f["alphabetLength"].max() == 20
        _check(b, checker, reads, [target] * len(reads), mode, task, -1, what=("shared", mode, task))
        again = b.run()
        assert {k: again[k] for k in STATS} == {k: stats[k] for k in STATS}
        _same(b.results_flat(), f, "a second run")
    finally:
        b.close()
