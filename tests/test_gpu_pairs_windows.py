"""GPU: pairs gathered from a window batch (edlibAmdBatchPairsSetWindows, PairBatch.set_windows): after set_windows + run()
a resident pair batch must be exactly a fresh PairBatch created over the same pairs materialised on the host -- every
array of results_flat(), both CIGAR forms and the statistics that describe the work -- and a strided sample (or all) of
its units must equal the checker; the window batch must be left as it was; a refused call must leave the pair batch as
it was.  The yardstick and its helpers are in tests/pairs_set_cases.py.
Two refusals of the contract have no case here: a window batch left without units by a SetUnits that failed on the device
(only a device error, out of memory, gets there, and no test provokes one), and batches on different devices (checked
where the machine has a second device, a branch a one-device machine does not take)."""
import functools

import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth
import pairs_set_cases as PS
from pairs_set_cases import (IUPAC, STATS, Tuples, check as _check, fresh as _fresh, mapper_tuples as _mapper_tuples,
                             reads as _reads, same as _same, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

NAME = "edlibAmdBatchPairsSetWindows"
QUERY_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 150, 255, 256)

# ---- the yardstick and the tuples of tests/pairs_set_cases.py, over a window batch

_set_and_compare = functools.partial(PS.set_and_compare, "set_windows")
_refused = functools.partial(PS.refused, NAME)
# the grid of tests/test_pairs_gather_model.py: every nibble phase x every window length
_grid = functools.partial(PS.grid, phases=8)


@pytest.fixture(scope="module")
def genome():
    """a 20,000-base ACGT target, 400 reads of 30 to 256 bases from both of its strands, and a window batch over them"""
    return PS.genome(2024, 11)


def _window_batch(engine, genome, stranded, mode="HW", k=-1):
    """a window batch over the reads: one unit per read at its locus (on its strand where stranded)"""
    n = len(genome["reads"])
    m = np.array([len(r) for r in genome["reads"]])
    s = np.maximum(genome["origin"] - 10, 0)
    e = np.minimum(genome["origin"] + m + 10, len(genome["target"]))
    return engine.WindowBatch(genome["reads"], genome["target"], np.arange(n), s, e - s, mode=mode, k=k,
                              unit_strand=genome["strand"] if stranded else None)


# ---- 1. modes, tasks, thresholds

@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("task", ["distance", "locations", "path"])
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_set_windows_equals_fresh_batch(engine, checker, genome, mode, task, k):
    rng = np.random.default_rng(["NW", "SHW", "HW"].index(mode) * 100 + ["distance", "locations", "path"].index(task) * 10 + k + 1)
    stranded = (k == 5)                                  # the source pool: plain (strand 1 made on the fly) or stranded
    wb = _window_batch(engine, genome, stranded)
    pb = engine.PairBatch([], [], mode=mode, task=task, k=k)
    try:
        tup = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), 2000, mode)
        assert tup.st.any() and not tup.st.all()
        got, stats = _set_and_compare(engine, checker, pb, wb, genome["reads"], genome["target"], tup, mode, task, k,
                                      what=(mode, task, k))
        assert stats["path"] & 2 and (got["editDistance"] >= 0).any()
        if k >= 0:
            assert (got["editDistance"] == -1).any()
    finally:
        pb.close()
        wb.close()


# ---- 2. the shapes the gather can get wrong

@pytest.mark.parametrize("alphabet", [b"ACGT", b"ACGTNacgtn", b"ACGTRYKMBDHVNSWU", b"A"])
@pytest.mark.parametrize("stranded", [False, True])
def test_phase_length_alignment_grid(engine, checker, alphabet, stranded):
    """a few hundred pairs, every unit against the checker; targets of 1, 4, 10 (N and lower case) and 16 symbols; queries
    of the lengths around the word and run sizes with IUPAC codes, lower case and U, on both strands"""
    rng = np.random.default_rng(len(alphabet) + 10 * stranded)
    A = np.frombuffer(alphabet, dtype=np.uint8)
    Q = np.frombuffer(b"ACGTNacgtnUuRYKMBVDHSW", dtype=np.uint8)
    target = A[rng.integers(0, len(A), size=5003)].tobytes()
    queries = [Q[rng.integers(0, len(Q), size=m)].tobytes() for m in QUERY_LENGTHS]
    nq = len(queries)
    wb = engine.WindowBatch(queries, target, np.arange(nq), np.zeros(nq), np.full(nq, 100), mode="HW",
                            unit_strand=(np.arange(nq) & 1) if stranded else None)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        tup = _grid(rng, len(target), nq)
        got, _ = _set_and_compare(engine, checker, pb, wb, queries, target, tup, "HW", "path", -1, everything=True,
                                  what=("grid", alphabet, stranded))
        assert got["alphabetLength"].max() >= len(alphabet)
        order = rng.permutation(len(tup))                # the same pairs in another order: every boundary elsewhere
        tup2 = Tuples(tup.q[order], tup.s[order], tup.n[order], tup.st[order])
        _set_and_compare(engine, checker, pb, wb, queries, target, tup2, "HW", "path", -1, everything=True, what="permuted")
        # a NULL strand array is all forward
        _set_and_compare(engine, checker, pb, wb, queries, target, Tuples(tup.q, tup.s, tup.n), "HW", "path", -1,
                         everything=True, what="forward")
    finally:
        pb.close()
        wb.close()


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025])
def test_counts(engine, checker, genome, n):
    rng = np.random.default_rng(300 + n)
    wb = _window_batch(engine, genome, False)
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    try:
        big = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), 1500, "HW")
        _set_and_compare(engine, checker, pb, wb, genome["reads"], genome["target"], big, "HW", "locations", -1, what="before")
        tup = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), n, "HW")
        got, stats = _set_and_compare(engine, checker, pb, wb, genome["reads"], genome["target"], tup, "HW", "locations", -1,
                                      everything=n < 1024, what=n)
        assert len(got["editDistance"]) == n and stats["path"] == (2 if n else 0), (n, stats)
    finally:
        pb.close()
        wb.close()


@pytest.mark.parametrize("task", ["distance", "path"])
def test_a_window_of_65536_columns(engine, checker, task):
    rng = np.random.default_rng(65536)
    target = synth.random_dna(3, 70001).tobytes()
    reads, origin, strand = _reads(rng, target, 50, 60, 200)
    wb = engine.WindowBatch(reads, target, np.arange(50), origin, [len(r) for r in reads], mode="HW")
    pb = engine.PairBatch([], [], mode="HW", task=task)
    try:
        tup = _mapper_tuples(rng, reads, origin, strand, len(target), 1100, "HW")
        tup.s[500], tup.n[500] = 4465, 65536
        tup.s[0], tup.n[0] = 0, 65536
        _set_and_compare(engine, checker, pb, wb, reads, target, tup, "HW", task, -1, what="65536")
        qs, ts = tup.materialise(reads, target)
        _check(pb, checker, qs, ts, "HW", task, -1, sel=(0, 500), what="65536")
    finally:
        pb.close()
        wb.close()


def test_a_window_of_65537_columns_is_refused(engine, checker):
    rng = np.random.default_rng(65537)
    target = synth.random_dna(3, 70001).tobytes()
    reads, origin, strand = _reads(rng, target, 50, 60, 200)
    wb = engine.WindowBatch(reads, target, np.arange(50), origin, [len(r) for r in reads], mode="HW")
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        tup = _mapper_tuples(rng, reads, origin, strand, len(target), 1100, "HW")
        pb.set_windows(wb, *tup.args())
        pb.run()
        before = _snapshot(pb)
        tup.s[3], tup.n[3] = 4464, 65537
        _refused(engine, pb, before,
                 lambda: engine.lib().edlibAmdBatchPairsSetWindows(pb._h, wb._h, tup.q.ctypes.data, tup.s.ctypes.data,
                                                                    tup.n.ctypes.data, tup.st.ctypes.data, len(tup)),
                 "pair 3", "65,537", "65,536", "create a new batch")
    finally:
        pb.close()
        wb.close()


def test_query_offsets_of_the_window_batch_need_not_start_at_zero(engine, checker, genome):
    """edlibAmdBatchWindowsSetUnits over a pool with bytes in front of the first query: the gathered set is planned from
    the differences of the offsets the window batch keeps"""
    rng = np.random.default_rng(37)
    reads, target = genome["reads"], genome["target"]
    n = len(reads)
    wb = _window_batch(engine, genome, False)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        lead = 37
        pool = np.frombuffer(b"x" * lead + b"".join(reads) + b"\0", dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        off += lead
        uq = np.arange(n, dtype=np.int32)
        us = np.maximum(genome["origin"] - 10, 0).astype(np.int32)
        ul = np.full(n, 40, dtype=np.int32)
        st = genome["strand"].astype(np.uint8)
        for strands in (None, st):
            assert engine.lib().edlibAmdBatchWindowsSetUnits(wb._h, pool.ctypes.data, off.ctypes.data, n, uq.ctypes.data,
                                                             us.ctypes.data, ul.ctypes.data,
                                                             None if strands is None else strands.ctypes.data, n) == 0, engine.last_error()
            tup = _mapper_tuples(rng, reads, genome["origin"], genome["strand"], len(target), 1100, "HW")
            _set_and_compare(engine, checker, pb, wb, reads, target, tup, "HW", "path", -1, what=("lead 37", strands is None))
    finally:
        pb.close()
        wb.close()


# ---- 3. the states of the source, and the source stays as it was

def _window_views(wb):
    return {**wb.units(), **wb.best()}


def test_source_states_and_the_source_is_untouched(engine, checker, genome):
    rng = np.random.default_rng(401)
    reads, target = genome["reads"], genome["target"]
    L = len(target)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    wb = _window_batch(engine, genome, False)
    twin = _window_batch(engine, genome, False)           # never a source: what the source's own Run must still give
    try:
        twin.run()
        want = _window_views(twin)

        def tuples():
            return _mapper_tuples(rng, reads, genome["origin"], genome["strand"], L, 1200, "HW")

        # before its first Run: the views still fail afterwards, and its first Run is the twin's
        _set_and_compare(engine, checker, pb, wb, reads, target, tuples(), "HW", "path", -1, what="plain, no run yet")
        with pytest.raises(RuntimeError, match="Run it first"):
            wb.units()
        wstats = wb.run()
        _same(_window_views(wb), want, "the first run after a gather")
        # after a Run: the views held across the call, the views fetched afterwards, the next Run and its statistics
        held = {**wb.units(copy=False), **wb.best(copy=False)}
        _set_and_compare(engine, checker, pb, wb, reads, target, tuples(), "HW", "path", -1, what="plain, after a run")
        _same(held, want, "views held across the gather")
        _same(_window_views(wb), want, "views after the gather")
        del held
        again = wb.run()
        _same(_window_views(wb), want, "the next run")
        assert {f: again[f] for f in STATS} == {f: wstats[f] for f in STATS}

        # a stranded set through the same batch, a plain one again: the pool changes its layout under the gather
        n = len(reads)
        m = np.array([len(r) for r in reads])
        s = np.maximum(genome["origin"] - 10, 0)
        e = np.minimum(genome["origin"] + m + 10, L)
        for state, st in (("stranded set_units", genome["strand"]), ("plain set_units", None)):
            wb.set_units(reads, np.arange(n), s, e - s, unit_strand=st)
            _set_and_compare(engine, checker, pb, wb, reads, target, tuples(), "HW", "path", -1, what=(state, "no run yet"))
            wb.run()
            before = _window_views(wb)
            _set_and_compare(engine, checker, pb, wb, reads, target, tuples(), "HW", "path", -1, what=(state, "after a run"))
            _same(_window_views(wb), before, (state, "views after the gather"))
            wb.run()
            _same(_window_views(wb), before, (state, "the next run"))
        _same(before, want, "a plain set again")
    finally:
        pb.close()
        wb.close()
        twin.close()


def test_a_batch_created_stranded(engine, checker, genome):
    rng = np.random.default_rng(402)
    wb = _window_batch(engine, genome, True)
    pb = engine.PairBatch([], [], mode="NW", task="path")
    try:
        wb.run()
        before = _window_views(wb)
        tup = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), 1300, "NW")
        _set_and_compare(engine, checker, pb, wb, genome["reads"], genome["target"], tup, "NW", "path", -1, what="stranded")
        wb.run()
        _same(_window_views(wb), before, "the next run")
    finally:
        pb.close()
        wb.close()


# ---- 4. independence, chaining, configuration

def test_the_pair_batch_outlives_the_window_batch(engine, checker, genome):
    rng = np.random.default_rng(403)
    reads, target = genome["reads"], genome["target"]
    wb = _window_batch(engine, genome, False)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        tup = _mapper_tuples(rng, reads, genome["origin"], genome["strand"], len(target), 1200, "HW")
        pb.set_windows(wb, *tup.args())
        wb.close()
        edlib_amd.lib().edlibAmdTrim()                    # the window batch's blocks go back to the driver
        pb.run()
        qs, ts = tup.materialise(reads, target)
        want, _ = _fresh(engine, qs, ts, "HW", "path", -1)
        _same(_snapshot(pb), want, "after the window batch closed")
        with pytest.raises(RuntimeError, match=NAME):
            pb.set_windows(wb, *tup.args())               # a closed batch is a NULL handle
        pb.run()
        _same(_snapshot(pb), want, "after the refusal")
    finally:
        pb.close()
        wb.close()


def test_set_pairs_and_set_windows_on_one_batch(engine, checker, genome):
    rng = np.random.default_rng(404)
    reads, target = genome["reads"], genome["target"]
    wb = _window_batch(engine, genome, False)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        for c in range(2):
            tup = _mapper_tuples(rng, reads, genome["origin"], genome["strand"], len(target), 1100 + 100 * c, "HW")
            _set_and_compare(engine, checker, pb, wb, reads, target, tup, "HW", "path", -1, what=("windows", c))
            other = _mapper_tuples(rng, reads, genome["origin"], genome["strand"], len(target), 1300, "HW")
            qs, ts = other.materialise(reads, target)
            pb.set_pairs(qs, ts)
            pb.run()
            want, _ = _fresh(engine, qs, ts, "HW", "path", -1)
            _same(_snapshot(pb), want, ("pairs", c))
    finally:
        pb.close()
        wb.close()


@pytest.mark.parametrize("mode,task", [("HW", "locations"), ("NW", "path")])
def test_the_pair_batch_keeps_its_own_equalities(engine, checker, mode, task):
    rng = np.random.default_rng(405)
    T = np.frombuffer(b"ACGTN", dtype=np.uint8)
    Q = np.frombuffer(b"ACGTRY", dtype=np.uint8)
    target = T[rng.integers(0, 5, size=20000)].tobytes()
    reads, origin, strand = _reads(rng, target, 300, 30, 200, sub=0.02)
    # (queries with codes the target does not hold: R and Y match by the pair batch's list alone)
    reads = [bytes(Q[rng.integers(0, 6)] if rng.random() < 0.05 else c for c in r) for r in reads]
    wb = engine.WindowBatch(reads, target, np.arange(300), origin, [len(r) for r in reads], mode="HW")    # no equalities
    pb = engine.PairBatch([], [], mode=mode, task=task, additionalEqualities=IUPAC)
    try:
        tup = _mapper_tuples(rng, reads, origin, strand, len(target), 1150, mode)
        _set_and_compare(engine, checker, pb, wb, reads, target, tup, mode, task, -1, eqs=IUPAC, what=(mode, task))
    finally:
        pb.close()
        wb.close()


# ---- 5. refusals leave the pair batch as it was

@pytest.mark.parametrize("mode", ["HW", "NW"])
def test_refusals_leave_the_pair_batch_as_it_was(engine, checker, genome, mode):
    rng = np.random.default_rng(501)
    reads, target = list(genome["reads"]), genome["target"]
    reads[7] = b""                                        # (a window batch takes an empty query; a streamed pair set does not)
    reads[8] = b"ACGT" * 64                               # 256 bases
    L = len(target)
    n = len(reads)
    wb = engine.WindowBatch(reads, target, np.arange(n), np.zeros(n), np.full(n, 300), mode="HW")
    first = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], L, 1200, mode)
    first.q[first.q == 7] = 9
    pb = engine.PairBatch([], [], mode=mode, task="path")
    lib = engine.lib()
    try:
        pb.set_windows(wb, *first.args())
        pb.run()
        before = _snapshot(pb)
        ok = Tuples([1, 2, 3, 4], [10, 20, 30, 40], [200, 210, 220, 230], [0, 1, 0, 1])

        def raw(windows, q, s, ln, st, count):
            ptr = lambda a: None if a is None else a.ctypes.data
            return lib.edlibAmdBatchPairsSetWindows(pb._h, None if windows is None else windows._h, ptr(q), ptr(s), ptr(ln),
                                                    ptr(st), count)

        def refused(call, *words):
            _refused(engine, pb, before, call, *words)

        def with_pair(at, q=None, s=None, ln=None, st=None):
            t = Tuples(ok.q.copy(), ok.s.copy(), ok.n.copy(), ok.st.copy())
            for arr, v in ((t.q, q), (t.s, s), (t.n, ln), (t.st, st)):
                if v is not None:
                    arr[at] = v
            return lambda: raw(wb, t.q, t.s, t.n, t.st, len(t))

        refused(lambda: raw(None, ok.q, ok.s, ok.n, ok.st, 4), "null", "window batch")
        refused(lambda: raw(wb, ok.q, ok.s, ok.n, ok.st, -1), "numPairs", "-1")
        refused(lambda: raw(wb, None, ok.s, ok.n, ok.st, 4), "NULL")
        refused(lambda: raw(wb, ok.q, None, ok.n, ok.st, 4), "NULL")
        refused(lambda: raw(wb, ok.q, ok.s, None, None, 4), "NULL")
        refused(with_pair(2, q=n), "pair 2", "query %d" % n, "numQueries = %d" % n)
        refused(with_pair(1, q=-1), "pair 1", "query -1")
        refused(with_pair(3, s=-5), "pair 3", "negative pairStart", "-5")
        refused(with_pair(0, ln=-2), "pair 0", "negative pairLength", "-2")
        refused(with_pair(2, s=L - 100, ln=101), "pair 2", "past the target", str(L - 100), "101", str(L))
        refused(with_pair(3, st=2), "pair 3", "pairStrand 2")
        refused(with_pair(1, q=7), "pair 1", "empty query", "create a new batch")
        refused(with_pair(2, ln=0), "pair 2", "empty target", "create a new batch")
        if mode == "NW":
            # the linear-space regime: (20 blocks + 8) T >= 1 MiB
            refused(with_pair(1, q=8, s=0, ln=12000), "pair 1", "256", "12,000", "linear-space", "create a new batch")
        # the caps of a set with paths, decided on the host from the lengths alone (nothing is allocated for a refused set):
        # the column stores, 64 bytes per column and block row of every pair's window (HW: of 2 m + 1 columns), above 32 GB
        w = 513 if mode == "HW" else 11900                # (NW: 256 x 11,900 stays below the 1 MiB rule)
        at = 2 ** 35 // (64 * (w + 4))                    # the pair that passes the cap
        many = np.zeros(at + 3, dtype=np.int32)
        refused(lambda: raw(wb, many + 8, many, many + (770 if mode == "HW" else w), None, len(many)),
                "pair %d" % at, "column stores", "32 GB", "EDLIB_TASK_PATH", "create a new batch")
        if mode == "HW":
            # ... and the op slots, m + window + 8 bytes a pair, above 8 GB: 256-base queries in one-column windows pass it
            # before their stores pass theirs -- 32.4 M tuples, the one heavy host pass of this file
            at = 2 ** 33 // (256 + 1 + 8)
            many = np.zeros(at + 3, dtype=np.int32)
            refused(lambda: raw(wb, many + 8, many, many + 1, None, len(many)),
                    "pair %d" % at, "op slots", "8 GB", "EDLIB_TASK_PATH", "create a new batch")
        del many
        # sources that have nothing resident
        A = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
        protein = A[rng.integers(0, 20, size=2000)].tobytes()
        wide = engine.WindowBatch([protein[5:60]], protein, [0], [0], [300], mode="HW")
        hosted = engine.WindowBatch([target[100:400], target[50:90]], target, [0, 1], [90, 40], [320, 60], mode="HW")
        try:
            z = np.zeros(1, dtype=np.int32)
            refused(lambda: raw(wide, z, z, z + 50, None, 1), "20 distinct symbols", "16")
            refused(lambda: raw(hosted, z + 1, z + 40, z + 60, None, 1), "host route", "edlibAmdBatchWindowsSetUnits")
            # ... until a set_units puts a set on the device
            hosted.set_units([target[50:90]], [0], [40], [60])
            assert raw(hosted, z, z + 40, z + 60, None, 1) == 0, engine.last_error()
            pb.n = 1
            pb.run()
            _check(pb, checker, [target[50:90]], [target[40:100]], mode, "path", -1, what="after set_units")
        finally:
            wide.close()
            hosted.close()
        if engine.device_count() > 1:
            far = engine.WindowBatch(reads[:2], target, [0, 1], [0, 0], [300, 300], mode="HW", device=1)
            try:
                assert raw(far, ok.q, ok.s, ok.n, ok.st, 4) != 0
                assert NAME in engine.last_error() and "device 1" in engine.last_error(), engine.last_error()
            finally:
                far.close()
        # a set that is taken still goes through
        _set_and_compare(engine, checker, pb, wb, reads, target, first, mode, "path", -1, what="after the refusals")
    finally:
        pb.close()
        wb.close()


def test_other_kinds_of_batch_are_refused_by_name(engine, genome):
    reads = [b"ACGTACGTAC", b"TTGACCA"]
    target = genome["target"][:400]
    z = np.zeros(2, dtype=np.int32)
    wb = engine.WindowBatch(reads, target, z, z, z + 50)
    pairs = engine.PairBatch(reads, [target, target], mode="HW", task="locations")
    lib = engine.lib()
    try:
        pairs.run()
        before = pairs.results_flat()
        as_pairs = [
            (lambda: engine.SharedBatch(reads, target), "a shared-target read batch"),
            (lambda: engine.CrossBatch(reads, [target]), "a cross batch"),
            (lambda: engine.SelfBatch(reads), "a self batch"),
            (lambda: engine.WindowBatch(reads, target, z, z, z + 50), "a window batch"),
        ]
        for make, kind in as_pairs:
            b = make()
            try:
                b.run()
                assert lib.edlibAmdBatchPairsSetWindows(b._h, wb._h, z.ctypes.data, z.ctypes.data, (z + 50).ctypes.data,
                                                        None, 2) != 0
                msg = engine.last_error()
                assert NAME in msg and kind in msg, msg
                b.run()                                   # the batch is what it was
            finally:
                b.close()
        assert lib.edlibAmdBatchPairsSetWindows(None, wb._h, z.ctypes.data, z.ctypes.data, (z + 50).ctypes.data, None, 2) != 0
        assert NAME in engine.last_error() and "null pair batch" in engine.last_error(), engine.last_error()
        as_windows = [
            (lambda: engine.PairBatch(reads, [target, target]), "a pair batch"),
            (lambda: engine.CrossBatch(reads, [target]), "a cross batch"),
        ]
        for make, kind in as_windows:
            b = make()
            try:
                assert lib.edlibAmdBatchPairsSetWindows(pairs._h, b._h, z.ctypes.data, z.ctypes.data, (z + 50).ctypes.data,
                                                        None, 2) != 0
                msg = engine.last_error()
                assert NAME in msg and kind in msg and "window batch" in msg, msg
                pairs.run()
                _same(pairs.results_flat(), before, kind)
            finally:
                b.close()
    finally:
        pairs.close()
        wb.close()
