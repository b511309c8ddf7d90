"""GPU: pairs gathered from a window batch (edlibAmdBatchPairsSetWindows, PairBatch.set_windows): after set_windows + run()
a resident pair batch must be exactly a fresh PairBatch created over the same pairs materialised on the host -- every
array of results_flat(), both CIGAR forms and the statistics that describe the work -- and a strided sample (or all) of
its units must equal the checker; the window batch must be left as it was; a refused call must leave the pair batch as
it was.  The yardstick and its helpers are those of tests/test_gpu_pairs_stream.py.
Two refusals of the contract have no case here: a window batch left without units by a SetUnits that failed on the device
(only a device error, out of memory, gets there, and no test provokes one), and batches on different devices (checked
where the machine has a second device, a branch a one-device machine does not take)."""
import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth

pytestmark = pytest.mark.gpu

NAME = "edlibAmdBatchPairsSetWindows"
STATS = ("cells", "word_steps", "path", "scan_launches")
FIELDS = ("status", "editDistance", "endLocations", "startLocations", "numLocations", "alignment", "alignmentLength",
          "alphabetLength")
IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]
WINDOW_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 400)
QUERY_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 150, 255, 256)


# ---- the yardstick of tests/test_gpu_pairs_stream.py

def _snapshot(b):
    """everything a caller can read after a run: results_flat() and both CIGAR forms"""
    out = dict(b.results_flat())
    for ext in (True, False):
        chars, off = b.cigars(extended=ext)
        out["cigar%d.chars" % ext], out["cigar%d.off" % ext] = chars, off
    return out


def _same(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for f in want:
        if want[f] is None or got[f] is None:
            assert got[f] is None and want[f] is None, (what, f)
            continue
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())


def _fresh(engine, qs, ts, mode, task, k, eqs=None):
    b = engine.PairBatch(qs, ts, mode=mode, task=task, k=k, additionalEqualities=eqs)
    try:
        stats = b.run()
        return _snapshot(b), stats
    finally:
        b.close()


def _check(b, checker, qs, ts, mode, task, k, eqs=None, sel=None, what=""):
    got = b.results(raw=True)
    assert len(got) == len(qs)
    bad = []
    for i in (range(len(qs)) if sel is None else sel):
        want = checker.align(qs[i], ts[i], mode, task, k, eq_pairs=eqs)
        if any(got[i][f] != want[f] for f in FIELDS):
            bad.append((i, len(qs[i]), len(ts[i]), {f: (got[i][f], want[f]) for f in FIELDS if got[i][f] != want[f]}))
    assert not bad, (what, mode, task, k, bad[:3])


# ---- sets over a window batch

class Tuples:
    """(query, start, length, strand) per pair, as set_windows takes them"""

    def __init__(self, q, s, n, st=None):
        self.q, self.s, self.n = (np.asarray(a, dtype=np.int32) for a in (q, s, n))
        self.st = None if st is None else np.asarray(st, dtype=np.uint8)

    def __len__(self):
        return len(self.q)

    def args(self):
        return self.q, self.s, self.n, self.st

    def materialise(self, queries, target):
        """the pairs on the host: slices of the target, reverse complements of the queries of strand 1"""
        t = bytes(target)
        qs = [bytes(queries[q]) if (self.st is None or not self.st[i]) else edlib_amd.reverse_complement(bytes(queries[q]))
              for i, q in enumerate(self.q)]
        return qs, [t[s:s + n] for s, n in zip(self.s, self.n)]


def _reads(rng, target, count, lo=30, hi=256, sub=0.03):
    """reads cut from the target with a few substitutions and now and then an indel, every other one from the reverse
    strand; where each came from"""
    t = np.frombuffer(bytes(target), dtype=np.uint8)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads, origin, strand = [], [], []
    for i, m in enumerate(rng.integers(lo, hi + 1, size=count)):
        m = int(m)
        s = int(rng.integers(0, len(t) - m + 1))
        q = t[s:s + m].copy()
        at = rng.integers(0, m, size=rng.binomial(m, sub))
        q[at] = A[rng.integers(0, 4, size=len(at))]
        if m > 4 and rng.random() < 0.3:
            p = int(rng.integers(1, m - 1))
            q = np.concatenate([q[:p], q[p + 1:], A[rng.integers(0, 4, size=1)]])
        st = i & 1
        reads.append(edlib_amd.reverse_complement(q.tobytes()) if st else q.tobytes())
        origin.append(s)
        strand.append(st)
    return reads, np.array(origin), np.array(strand)


def _mapper_tuples(rng, reads, origin, strand, target_length, n, mode):
    """n pairs in no order: a read in the strand it maps on (now and then the other one), its window around where it came
    from -- NW: about the read's span, SHW: from its first column on, HW: padded on both sides up to about 3 m; windows of
    reads from nearby loci overlap"""
    q = rng.integers(0, len(reads), size=n)
    m = np.array([len(reads[i]) for i in q], dtype=np.int64)
    st = np.where(rng.random(n) < 0.9, strand[q], 1 - strand[q])
    if mode == "NW":
        lead, trail = rng.integers(0, 3, size=n), rng.integers(0, 3, size=n)
    elif mode == "SHW":
        lead, trail = np.zeros(n, dtype=np.int64), rng.integers(0, 2 * m + 1)
    else:
        lead, trail = rng.integers(0, m + 1), rng.integers(0, m + 1)
    s = np.maximum(origin[q] - lead, 0)
    e = np.minimum(origin[q] + m + trail, target_length)
    return Tuples(q, s, e - s, st)


def _set_and_compare(engine, checker, pb, wb, queries, target, tup, mode, task, k, eqs=None, everything=False, what=""):
    """set_windows + run on pb against a fresh batch over the materialised pairs, and about 100 units (or all) against
    the checker"""
    pb.set_windows(wb, *tup.args())
    assert pb.n == len(tup)
    stats = pb.run()
    got = _snapshot(pb)
    qs, ts = tup.materialise(queries, target)
    want, wstats = _fresh(engine, qs, ts, mode, task, k, eqs)
    _same(got, want, what)
    # (a fresh batch of fewer than 1,024 pairs takes the general path, whose word_steps and launches are another count:
    # there the statistics are those of the batch set_pairs makes)
    if len(tup) < 1024:
        other = engine.PairBatch([], [], mode=mode, task=task, k=k, additionalEqualities=eqs)
        try:
            other.set_pairs(qs, ts)
            wstats = other.run()
            _same(got, _snapshot(other), ("set_pairs", what))
        finally:
            other.close()
    assert {f: stats[f] for f in STATS} == {f: wstats[f] for f in STATS}, what
    assert stats["cells"] == sum(len(q) * len(t) for q, t in zip(qs, ts)), what
    n = len(qs)
    _check(pb, checker, qs, ts, mode, task, k, eqs, None if everything else range(0, n, max(1, n // 100)), what)
    return got, stats


@pytest.fixture(scope="module")
def genome():
    """a 20,000-base ACGT target, 400 reads of 30 to 256 bases from both of its strands, and a window batch over them"""
    rng = np.random.default_rng(2024)
    target = synth.random_dna(11, 20000).tobytes()
    reads, origin, strand = _reads(rng, target, 400)
    return {"target": target, "reads": reads, "origin": origin, "strand": strand}


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

def _grid(rng, target_length, num_queries):
    """the grid of tests/test_pairs_gather_model.py: every nibble phase x every window length, consecutive odd lengths
    (every alignment of the next pair), windows at column 0 and up to the last column, both strands"""
    ps, pl = [], []
    for phase in range(8):
        for n in WINDOW_LENGTHS:
            ps.append(8 * int(rng.integers(0, (target_length - 400) // 8 - 1)) + phase)
            pl.append(n)
    for n in range(1, 35, 2):
        ps.append(int(rng.integers(0, target_length - 40)))
        pl.append(n)
    for n in WINDOW_LENGTHS:
        ps += [0, target_length - n]
        pl += [n, n]
    pq = [i % num_queries for i in range(len(ps))]
    st = [(i // num_queries) & 1 for i in range(len(ps))]
    return Tuples(pq, ps, pl, st)


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

def _refused(engine, pb, before, call, *words):
    """the call fails with a message that names the function and carries `words`; the views held across it, the views
    fetched after it and the next Run are those of `before`"""
    held = pb.results_flat(copy=False)                    # views of the batch's own memory, held across the refusal
    cig = pb.cigars(copy=False)
    assert call() != 0
    msg = engine.last_error()
    assert NAME in msg and all(w in msg for w in words), msg
    for f, v in held.items():
        assert v is None or np.array_equal(v, before[f]), (msg, f)
    assert np.array_equal(cig[0], before["cigar1.chars"]) and np.array_equal(cig[1], before["cigar1.off"]), msg
    _same(_snapshot(pb), before, msg)
    del held, cig
    pb.run()                                              # ... and the next Run reproduces them
    _same(_snapshot(pb), before, ("the next run", msg))


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
