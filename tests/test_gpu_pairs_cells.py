"""GPU: pairs gathered from a cross or self batch (edlibAmdBatchPairsSetCells, PairBatch.set_cells): after set_cells +
run() a resident pair batch must be exactly a fresh PairBatch created over the same pairs materialised on the host --
every array of results_flat(), both CIGAR forms and the statistics that describe the work -- and a strided sample (or
all) of its units must equal the checker; the source must be left as it was; a refused call must leave the pair batch as
it was; and hits(), cell_windows, set_cells, a locations Run must give the checker's whole-target HW answer of every hit.
The yardstick is tests/pairs_set_cases.py, the tuples and the sources are tests/pairs_cells_cases.py.
Two refusals of the contract have no case here: batches on different devices (a one-device machine), and a source left
without targets by a SetTargets that failed on the device (no test makes a device fail)."""
import functools

import numpy as np
import pytest

import edlib_amd
import pairs_set_cases as PS
import pairs_cells_cases as PC
from pairs_set_cases import IUPAC, STATS, WINDOW_LENGTHS
from pairs_cells_cases import CROSS_KINDS, KINDS, SELF_KINDS, CellTuples

pytestmark = pytest.mark.gpu

NAME = "edlibAmdBatchPairsSetCells"
MODES = ("NW", "SHW", "HW")
TASKS = ("distance", "locations", "path")

_same = functools.partial(PS.same, scalars=True)
_set_and_compare = functools.partial(PS.set_and_compare, "set_cells")
_refused = functools.partial(PS.refused, NAME)


@pytest.fixture(scope="module")
def data():
    """60 targets of 1 to 2,000 bases in the caller's order, 40 queries of 20 to 256 bases cut from them on both strands,
    and one of 300 bases that the cross kernel does not scan"""
    d = PC.related(np.random.default_rng(2026), 40, 60)
    d["queries"].append(bytes(d["targets"][3][100:400]))
    return d


# ---- 1. modes x tasks x k

@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("mode", MODES)
def test_set_cells_equals_fresh_batch(engine, checker, data, mode, task, k):
    seed = MODES.index(mode) * 10 + TASKS.index(task) + (100 if k < 0 else 0)
    rng = np.random.default_rng(seed)
    kind = ("cross", "hits", "both")[seed % 3]
    src = PC.source(engine, kind, data["queries"], data["targets"], mode=mode)
    pb = engine.PairBatch([], [], mode=mode, task=task, k=k)
    try:
        if seed % 2:
            src.run()                                       # (a source that has run, and one that has not)
        tup = PC.cell_tuples(rng, data, 1500, mode)
        if task == "path" and mode != "NW":                 # (a streamed SHW / HW set with paths: queries up to 256 bases)
            tup.q[tup.q == 40] = 7
        else:
            tup.q[:5] = 40
        assert tup.st.any() and not tup.st.all() and len(set(tup.t.tolist())) > 40
        got, stats = _set_and_compare(engine, checker, pb, src, data["queries"], data["targets"], tup, mode, task, k,
                                      what=(kind, mode, task, k))
        assert stats["path"] & 2 and (got["editDistance"] >= 0).any()
        if k >= 0:
            assert (got["editDistance"] == -1).any()
    finally:
        pb.close()
        src.close()


# ---- 2. the shapes the gather can get wrong

GRID_LENGTHS = (33, 1, 1031, 8, 2, 17, 7, 64, 9, 16, 15, 32, 31, 8, 400, 1031)
QUERY_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 150, 255, 256, 300, 1024)


def _grid(rng, targets):
    """every nibble phase of a window's first column x every window length (in the 1,031-base targets), every target
    whole, windows that end on every target's last base, both strands"""
    pt, ps, pl = [], [], []
    long_ones = [t for t in range(len(targets)) if len(targets[t]) == 1031]
    for phase in range(8):
        for n in WINDOW_LENGTHS:
            pt.append(long_ones[(phase + n) % 2])
            ps.append(phase + 8 * int(rng.integers(0, (1031 - n - phase) // 8 + 1)))
            pl.append(n)
    for t, seq in enumerate(targets):
        pt += [t, t]; ps += [0, len(seq) - 1]; pl += [len(seq), 1]
        for n in WINDOW_LENGTHS:
            if n < len(seq):
                pt.append(t); ps.append(len(seq) - n); pl.append(n)
    pq = [i % len(QUERY_LENGTHS) for i in range(len(pt))]
    st = [(i // len(QUERY_LENGTHS)) & 1 for i in range(len(pt))]
    return CellTuples(pq, pt, ps, pl, st)


@pytest.mark.parametrize("alphabet", [b"ACGT", b"ACGTNacgtn", b"ACGTRYKMSWBDHVN" + bytes([200]), b"A"])
def test_phase_length_grid(engine, checker, alphabet):
    """about 250 pairs over targets of the lengths around the dword and run sizes, every unit against the checker; targets
    of 4, 10, 16 (one byte >= 128) and 1 symbols; queries up to 1,024 bases, those of 300 and 1,024 outside the kernel"""
    rng = np.random.default_rng(len(alphabet))
    A = np.frombuffer(alphabet, dtype=np.uint8)
    Q = np.frombuffer(b"ACGTNacgtnUuRYKMBVDHSW", dtype=np.uint8)
    targets = []
    for n in GRID_LENGTHS:
        t = A[rng.integers(0, len(A), size=n)]
        t[::7] = A[-1]
        targets.append(t.tobytes())
    queries = [Q[rng.integers(0, len(Q), size=m)].tobytes() for m in QUERY_LENGTHS]
    src = engine.CrossBatch(queries, targets, mode="HW")
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    short = engine.PairBatch([], [], mode="HW", task="path")
    try:
        tup = _grid(rng, targets)
        assert 200 <= len(tup) <= 320
        got, _ = _set_and_compare(engine, checker, pb, src, queries, targets, tup, "HW", "locations", -1, everything=True,
                                  what=("grid", alphabet))
        assert got["alphabetLength"].max() >= len(alphabet)
        order = rng.permutation(len(tup))                # the same pairs in another order: every boundary elsewhere
        _set_and_compare(engine, checker, pb, src, queries, targets, tup.take(order), "HW", "locations", -1,
                         everything=True, what="permuted")
        # a NULL strand array is all forward
        _set_and_compare(engine, checker, pb, src, queries, targets, CellTuples(tup.q, tup.t, tup.s, tup.n), "HW",
                         "locations", -1, everything=True, what="forward")
        # with paths: the queries a streamed HW set with paths takes (up to 256 bases)
        nshort = sum(m <= 256 for m in QUERY_LENGTHS)
        _set_and_compare(engine, checker, short, src, queries, targets, CellTuples(tup.q % nshort, tup.t, tup.s, tup.n, tup.st),
                         "HW", "path", -1, everything=True, what="paths")
    finally:
        pb.close()
        short.close()
        src.close()


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025])
def test_counts(engine, checker, data, n):
    rng = np.random.default_rng(300 + n)
    src = PC.source(engine, "both", data["queries"], data["targets"])
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    try:
        big = PC.cell_tuples(rng, data, 1500, "HW")
        _set_and_compare(engine, checker, pb, src, data["queries"], data["targets"], big, "HW", "locations", -1, what="before")
        tup = PC.cell_tuples(rng, data, n, "HW")
        got, stats = _set_and_compare(engine, checker, pb, src, data["queries"], data["targets"], tup, "HW", "locations", -1,
                                      everything=n < 1024, what=n)
        assert len(got["editDistance"]) == n and stats["path"] == (2 if n else 0), (n, stats)
    finally:
        pb.close()
        src.close()


# ---- 3. every source kind, its states, and what it keeps

@pytest.mark.parametrize("kind", KINDS)
def test_every_source_kind_in_every_state_is_left_as_it_was(engine, checker, kind):
    """before any Run, after a Run and (cross kinds) after set_targets to another chunk, whose pack order is another one;
    strand 1 comes from the stranded pool of a both-strand source and is made on the fly from a plain one"""
    rng = np.random.default_rng(700 + KINDS.index(kind))
    own = kind in SELF_KINDS
    d = PC.related(rng, 50, 30, qlo=20, qhi=200, tlo=20 if own else 1, thi=256 if own else 900)
    if own:
        # one set: the sequences are the targets and some of the queries cut from them; both indices name sequences of it
        seqs = d["targets"] + d["queries"][:20]
        d = {"queries": seqs, "targets": seqs, "origin_t": np.zeros(0, dtype=np.int64), "origin_s": np.zeros(0, dtype=np.int64),
             "strand": np.zeros(0, dtype=np.int64)}
    mode = "NW" if own else "HW"
    make = lambda: PC.source(engine, kind, d["queries"], None if own else d["targets"], mode=mode, k=12)
    pb = engine.PairBatch([], [], mode=mode, task="path")
    src, twin = make(), make()                              # twin: never a source, what the source's own Run must still give
    try:
        tstats = twin.run()
        want = PC.source_views(twin, kind)

        def gather(what, n=1100):
            tup = PC.cell_tuples(rng, d, n, mode)
            if own:
                assert (tup.q > tup.t).any() and (tup.q < tup.t).any()
            _set_and_compare(engine, checker, pb, src, d["queries"], d["targets"], tup, mode, "path", -1, what=(kind, what))

        gather("no run yet")
        with pytest.raises(RuntimeError):
            PC.source_views(src, kind)
        stats = src.run()
        _same(PC.source_views(src, kind), want, "the first run after a gather")
        assert {f: stats[f] for f in STATS} == {f: tstats[f] for f in STATS}
        held = PC.source_views(src, kind, copy=False)
        gather("after a run")
        _same(held, want, "views held across the gather")
        _same(PC.source_views(src, kind), want, "views after the gather")
        del held
        again = src.run()
        _same(PC.source_views(src, kind), want, "the next run")
        assert {f: again[f] for f in STATS} == {f: tstats[f] for f in STATS}
        if not own:
            # another chunk: other lengths, so another order in the pack; the pairs come from it
            d2 = PC.related(rng, 50, 45, qlo=20, qhi=200, thi=700)
            d = dict(d2, queries=d["queries"], origin_t=np.zeros(0, dtype=np.int64))
            src.set_targets(d["targets"])
            twin.set_targets(d["targets"])
            gather("after set_targets", 300)
            tstats = twin.run()
            stats = src.run()
            _same(PC.source_views(src, kind), PC.source_views(twin, kind), "the run of the new chunk")
            assert {f: stats[f] for f in STATS} == {f: tstats[f] for f in STATS}
            gather("the new chunk after its run", 300)
    finally:
        pb.close()
        src.close()
        twin.close()


def test_whole_targets_of_the_pairs_within_k_of_a_self_batch(engine, checker):
    rng = np.random.default_rng(801)
    base = [DNA_random(rng, int(m)) for m in rng.integers(40, 120, size=12)]
    seqs = []
    for i in range(150):                                     # clusters: a few edits around twelve centres
        s = bytearray(base[i % 12])
        for _ in range(int(rng.integers(0, 4))):
            s[int(rng.integers(0, len(s)))] = b"ACGT"[int(rng.integers(0, 4))]
        seqs.append(bytes(s))
    src = engine.SelfBatch(seqs, k=6, hits=True)
    pb = engine.PairBatch([], [], mode="NW", task="path")
    try:
        src.run()
        hits = src.hits()
        first = np.repeat(np.arange(len(seqs)), np.diff(hits["rowOffsets"]))
        assert 300 < len(first) < 3000
        pb.set_cells(src, first, hits["partner"])            # start and length None: whole targets
        src.close()
        pb.run()
        qs, ts = PC.materialise(seqs, seqs, first, hits["partner"])
        PS.check(pb, checker, qs, ts, "NW", "path", -1, what="pairs within k")
        assert np.array_equal(pb.results_flat()["editDistance"], hits["editDistance"])
    finally:
        pb.close()
        src.close()


def DNA_random(rng, n):
    return PC.DNA[rng.integers(0, 4, size=n)].tobytes()


def test_the_pair_batch_outlives_the_source(engine, checker, data):
    rng = np.random.default_rng(802)
    src = PC.source(engine, "hits", data["queries"], data["targets"])
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        def gone():
            src.close()
            edlib_amd.lib().edlibAmdTrim()                   # its blocks go back to the driver

        tup = PC.cell_tuples(rng, data, 1200, "HW")
        tup.q[tup.q == 40] = 0
        _set_and_compare(engine, checker, pb, src, data["queries"], data["targets"], tup, "HW", "path", -1, what="closed",
                         before_run=gone)
        want = PS.snapshot(pb)
        with pytest.raises(RuntimeError, match=NAME):
            pb.set_cells(src, *tup.args())                   # a closed batch is a NULL handle
        pb.run()
        _same(PS.snapshot(pb), want, "after the refusal")
    finally:
        pb.close()
        src.close()


def test_set_pairs_and_set_cells_alternate_on_one_batch(engine, checker, data):
    rng = np.random.default_rng(803)
    src = PC.source(engine, "cross", data["queries"], data["targets"])
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    try:
        for c in range(2):
            tup = PC.cell_tuples(rng, data, 1100 + 100 * c, "HW")
            _set_and_compare(engine, checker, pb, src, data["queries"], data["targets"], tup, "HW", "locations", -1,
                             what=("cells", c))
            qs, ts = PC.cell_tuples(rng, data, 1300, "HW").materialise(data["queries"], data["targets"])
            pb.set_pairs(qs, ts)
            pb.run()
            want, _ = PS.fresh(engine, qs, ts, "HW", "locations", -1)
            _same(PS.snapshot(pb), want, ("pairs", c))
    finally:
        pb.close()
        src.close()


@pytest.mark.parametrize("mode,task", [("HW", "locations"), ("NW", "path")])
def test_the_pair_batch_keeps_its_own_equalities(engine, checker, mode, task):
    rng = np.random.default_rng(804)
    d = PC.related(rng, 60, 40, qlo=30, qhi=200, thi=900)
    N = np.frombuffer(b"ACGTN", dtype=np.uint8)
    Q = np.frombuffer(b"ACGTRY", dtype=np.uint8)
    # (targets with N, queries with codes the targets do not hold: they match by the pair batch's list alone)
    d["targets"] = [bytes(N[4] if rng.random() < 0.03 else c for c in t) for t in d["targets"]]
    d["queries"] = [bytes(Q[rng.integers(4, 6)] if rng.random() < 0.05 else c for c in q) for q in d["queries"]]
    src = engine.CrossBatch(d["queries"], d["targets"], mode="HW")        # no equalities
    pb = engine.PairBatch([], [], mode=mode, task=task, additionalEqualities=IUPAC)
    try:
        tup = PC.cell_tuples(rng, d, 1150, mode)
        _set_and_compare(engine, checker, pb, src, d["queries"], d["targets"], tup, mode, task, -1, eqs=IUPAC, what=(mode, task))
        plain, _ = PS.fresh(engine, *tup.materialise(d["queries"], d["targets"]), mode, task, -1)
        assert (plain["editDistance"] != PS.snapshot(pb)["editDistance"]).any()
    finally:
        pb.close()
        src.close()


# ---- 4. targets that are not in the pack

def test_a_65536_base_target_whole_and_a_longer_one_beside_it(engine, checker):
    rng = np.random.default_rng(805)
    targets = [DNA_random(rng, 500), DNA_random(rng, 65536), DNA_random(rng, 65537), DNA_random(rng, 90)]
    queries = [targets[1][1000:1100], targets[0][50:250], targets[2][7:300][:256]]
    src = engine.CrossBatch(queries, targets, mode="HW", k=20)
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    try:
        tup = CellTuples([0, 1, 2, 0, 1], [1, 0, 3, 1, 1], [0, 0, 0, 65536 - 9, 4465], [65536, 500, 90, 9, 61000], [0, 1, 0, 1, 0])
        _set_and_compare(engine, checker, pb, src, queries, targets, tup, "HW", "locations", -1, everything=True, what="65,536")
        before = PS.snapshot(pb)
        bad = CellTuples([0, 1, 2], [1, 2, 0], [0, 10, 0], [100, 100, 100])
        with pytest.raises(RuntimeError) as err:
            pb.set_cells(src, *bad.args())
        msg = str(err.value)
        assert NAME in msg and "pair 1" in msg and "target 2" in msg and "65,537" in msg and "not resident" in msg \
            and "edlibAmdBatchPairsSetPairs" in msg, msg
        pb.run()
        _same(PS.snapshot(pb), before, "after the refusal")
        src.run()                                           # its internal session and its kernel share still run
        assert src.matrix()["editDistance"][1, 0] == 0
        _set_and_compare(engine, checker, pb, src, queries, targets, tup.take(np.array([4, 2, 0])), "HW", "locations", -1,
                         everything=True, what="after a run")
    finally:
        pb.close()
        src.close()


@pytest.mark.parametrize("kind", ["cross", "self"])
def test_a_set_of_17_symbols_has_no_pack(engine, kind):
    rng = np.random.default_rng(806)
    A = np.arange(65, 82, dtype=np.uint8)
    seqs = [A[rng.integers(0, 17, size=120)].tobytes() for _ in range(6)]
    seqs[0] = A.tobytes() * 4
    src = engine.CrossBatch(seqs[:3], seqs, mode="NW") if kind == "cross" else engine.SelfBatch(seqs)
    pb = engine.PairBatch(seqs[:2], seqs[2:4], mode="NW", task="path")
    try:
        pb.run()
        before = PS.snapshot(pb)
        z = np.zeros(2, dtype=np.int32)
        _refused(engine, pb, before, lambda: engine.lib().edlibAmdBatchPairsSetCells(
            pb._h, src._h, z.ctypes.data, (z + 1).ctypes.data, None, None, None, 2),
            "pair 0", "target 1", "not resident", "edlibAmdBatchPairsSetPairs")
        assert pb.set_cells(src, [], []) is None and pb.n == 0           # no pairs: nothing to gather
    finally:
        pb.close()
        src.close()


def test_a_self_sequence_outside_the_kernel_is_refused_by_name(engine, checker):
    rng = np.random.default_rng(807)
    seqs = [DNA_random(rng, int(m)) for m in (100, 300, 120, 256, 90)]
    src = engine.SelfBatch(seqs)
    pb = engine.PairBatch([], [], mode="NW", task="path")
    try:
        # a query of 300 bases is in the pool; as a target it is not in the pack
        tup = CellTuples([1, 0, 3, 4], [0, 2, 4, 3])
        _set_and_compare(engine, checker, pb, src, seqs, seqs, tup, "NW", "path", -1, everything=True, what="self")
        with pytest.raises(RuntimeError) as err:
            pb.set_cells(src, [0, 2], [2, 1])
        assert NAME in str(err.value) and "pair 1" in str(err.value) and "target 1 (300 bases)" in str(err.value) \
            and "the self batch" in str(err.value), str(err.value)
    finally:
        pb.close()
        src.close()


# ---- 5. refusals leave the pair batch as it was

@pytest.mark.parametrize("mode", ["HW", "NW"])
def test_refusals_leave_the_pair_batch_as_it_was(engine, checker, mode):
    rng = np.random.default_rng(501)
    d = PC.related(rng, 60, 30, qlo=60, qhi=200, tlo=300, thi=2000)
    queries, targets = list(d["queries"]), list(d["targets"])
    good = list(queries)
    queries[7] = b""                                      # (a cross batch takes an empty query; a streamed pair set does not)
    queries[8] = b"ACGT" * 64                             # 256 bases
    queries[9] = bytes(targets[3][100:400])               # 300 bases: above a streamed SHW / HW set with paths
    queries[10] = bytes(targets[3][:1025])                # 1,025 bases: above any streamed set
    targets[5] = DNA_random(rng, 12100)
    targets[6] = DNA_random(rng, 70000)                   # not in the pack
    nq, nt = len(queries), len(targets)
    src = engine.CrossBatch(queries, targets, mode="HW")
    other = engine.PairBatch(good[:2], targets[:2])
    wb = engine.WindowBatch(good[:2], targets[0], [0, 1], [0, 0], [50, 50])
    pb = engine.PairBatch([], [], mode=mode, task="path")
    lib = engine.lib()
    try:
        d["queries"] = good
        first = PC.cell_tuples(rng, d, 1200, mode)
        first.q[(first.q >= 7) & (first.q <= 10)] = 11
        first.t[(first.t == 5) | (first.t == 6)] = 3
        first.s[first.t == 3] = 0
        first.n[first.t == 3] = 150
        pb.set_cells(src, *first.args())
        pb.run()
        before = PS.snapshot(pb)
        ok = CellTuples([1, 2, 3, 4], [0, 1, 2, 3], [10, 20, 30, 40], [200, 210, 220, 230], [0, 1, 0, 1])

        def raw(source, q, t, s, ln, st, count, pairs=pb):
            ptr = lambda a: None if a is None else a.ctypes.data
            return lib.edlibAmdBatchPairsSetCells(None if pairs is None else pairs._h, None if source is None else source._h,
                                                  ptr(q), ptr(t), ptr(s), ptr(ln), ptr(st), count)

        def refused(call, *words):
            _refused(engine, pb, before, call, *words)

        def with_pair(at, q=None, t=None, s=None, ln=None, st=None):
            c = CellTuples(ok.q.copy(), ok.t.copy(), ok.s.copy(), ok.n.copy(), ok.st.copy())
            for arr, v in ((c.q, q), (c.t, t), (c.s, s), (c.n, ln), (c.st, st)):
                if v is not None:
                    arr[at] = v
            return lambda: raw(src, c.q, c.t, c.s, c.n, c.st, len(c))

        refused(lambda: raw(None, *ok.args(), 4), "null cross batch")
        assert raw(src, *ok.args(), 4, pairs=None) != 0 and "null pair batch" in engine.last_error()
        refused(lambda: raw(other, *ok.args(), 4), "a pair batch", "cannot be gathered")
        refused(lambda: raw(wb, *ok.args(), 4), "a window batch", "cannot be gathered")
        assert raw(src, *ok.args(), 4, pairs=src) != 0
        assert NAME in engine.last_error() and "not available on a cross batch" in engine.last_error()
        refused(lambda: raw(src, *ok.args(), -1), "numPairs", "-1")
        refused(lambda: raw(src, None, ok.t, ok.s, ok.n, ok.st, 4), "NULL", "pairQuery")
        refused(lambda: raw(src, ok.q, None, ok.s, ok.n, ok.st, 4), "NULL", "pairTarget")
        refused(lambda: raw(src, ok.q, ok.t, None, ok.n, ok.st, 4), "pairStart", "NULL alone")
        refused(lambda: raw(src, ok.q, ok.t, ok.s, None, ok.st, 4), "pairLength", "NULL alone")
        refused(with_pair(2, q=nq), "pair 2", "query %d" % nq, "numQueries = %d" % nq, "cross batch")
        refused(with_pair(1, q=-1), "pair 1", "query -1")
        refused(with_pair(0, t=nt), "pair 0", "target %d" % nt, "numTargets = %d" % nt)
        refused(with_pair(3, t=-2), "pair 3", "target -2")
        refused(with_pair(3, s=-5), "pair 3", "negative pairStart", "-5")
        refused(with_pair(0, ln=-2), "pair 0", "negative pairLength", "-2")
        L2 = len(targets[2])
        refused(with_pair(2, s=L2 - 100, ln=101), "pair 2", "past target 2", str(L2 - 100), "101", str(L2))
        refused(with_pair(3, st=2), "pair 3", "pairStrand 2")
        refused(with_pair(1, t=6), "pair 1", "target 6", "70,000", "not resident", "edlibAmdBatchPairsSetPairs")
        refused(with_pair(1, q=7), "pair 1", "empty query", "create a new batch")
        refused(with_pair(2, ln=0), "pair 2", "empty target", "create a new batch")
        refused(with_pair(0, q=10), "pair 0", "1,025", "1,024", "create a new batch")
        if mode == "HW":
            refused(with_pair(1, q=9), "pair 1", "300", "256", "EDLIB_TASK_PATH", "HW", "create a new batch")
        else:
            # the linear-space regime: (20 blocks + 8) T >= 1 MiB
            refused(with_pair(1, q=8, t=5, s=0, ln=12000), "pair 1", "256", "12,000", "linear-space", "create a new batch")
        if engine.device_count() > 1:
            far = engine.CrossBatch(good[:2], targets[:2], mode="HW", device=1)
            try:
                assert raw(far, *ok.args(), 4) != 0
                assert NAME in engine.last_error() and "device 1" in engine.last_error(), engine.last_error()
            finally:
                far.close()
        # a set that is taken still goes through
        _set_and_compare(engine, checker, pb, src, queries, targets, first, mode, "path", -1, what="after the refusals")
    finally:
        pb.close()
        wb.close()
        other.close()
        src.close()


# ---- 6. end to end: hits within k, their windows, a locations Run

def test_barcode_hits_get_the_whole_reads_locations(engine, checker):
    rng = np.random.default_rng(77)
    barcodes = [DNA_random(rng, 24) for _ in range(16)]
    reads = []
    for i in range(3000):
        r = bytearray(DNA_random(rng, 150))
        if i % 10 != 3:                                   # (one read in ten carries no barcode)
            b = bytearray(barcodes[int(rng.integers(0, 16))])
            for _ in range(int(rng.integers(0, 4))):
                b[int(rng.integers(0, 24))] = b"ACGT"[int(rng.integers(0, 4))]
            at = int(rng.integers(0, 150 - 24 + 1)) if i % 7 else (0 if i % 2 else 126)
            r[at:at + 24] = b
        reads.append(bytes(r))
    src = engine.CrossBatch(barcodes, reads, mode="HW", k=3, hits=True)
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    try:
        src.run()
        hits = src.hits()
        target = np.repeat(np.arange(len(reads)), np.diff(hits["targetOffsets"]))
        kept, pq, pt, ps, pl, st = edlib_amd.cell_windows("HW", hits["query"], target, hits["editDistance"],
                                                          hits["endLocation"], [24] * 16, [150] * 3000)
        assert st is None and len(kept) == len(target) and 2600 <= len(kept) <= 3400
        pb.set_cells(src, pq, pt, ps, pl)
        src.close()
        pb.run()
        got = pb.results_flat()
        bad = []
        for i in range(len(kept)):
            want = checker.align(barcodes[pq[i]], reads[pt[i]], "HW", "locations", -1)
            lo = int(got["locOff"][i])
            mine = (int(got["editDistance"][i]), int(got["starts"][lo]) + int(ps[i]), int(got["ends"][lo]) + int(ps[i]))
            theirs = (want["editDistance"], want["startLocations"][0], want["endLocations"][0])
            if mine != theirs or mine[0] != hits["editDistance"][kept[i]]:
                bad.append((i, mine, theirs))
        assert not bad, bad[:5]
    finally:
        pb.close()
        src.close()
