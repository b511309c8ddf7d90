"""GPU: pairs gathered from a read batch (edlibAmdBatchPairsSetSharedWindows, PairBatch.set_shared_windows): after
set_shared_windows + run() a resident pair batch must be exactly a fresh PairBatch created over the same pairs
materialised on the host -- every array of results_flat(), both CIGAR forms and the statistics that describe the work --
and a strided sample (or all) of its units must equal the checker; the read batch must be left as it was; a refused call
must leave the pair batch as it was; and a distance Run, first_hit_windows, set_shared_windows, a path Run must give the
checker's whole-target HW path of every read that mapped.  The yardstick and its helpers are in
tests/pairs_set_cases.py.
One refusal of the contract has no case on a one-device machine: batches on different devices."""
import functools

import numpy as np
import pytest

import edlib_amd
from edlib_amd import synth
import pairs_set_cases as PS
from pairs_set_cases import (IUPAC, STATS, Tuples, check as _check, fresh as _fresh, mapper_tuples as _mapper_tuples,
                             reads as _reads, snapshot as _snapshot)

pytestmark = pytest.mark.gpu

NAME = "edlibAmdBatchPairsSetSharedWindows"
QUERY_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 150, 255, 256, 300, 1024)
KINDS = ("shared", "both", "hits")

# ---- the yardstick and the tuples of tests/pairs_set_cases.py, over a read batch

_same = functools.partial(PS.same, scalars=True)          # (the views of a hit-list source hold counts, too)
_set_and_compare = functools.partial(PS.set_and_compare, "set_shared_windows")
_refused = functools.partial(PS.refused, NAME)
# every source byte phase x every window length with the destination phase moving on (the lengths are odd and even):
# about 300 pairs
_grid = functools.partial(PS.grid, phases=4, reps=5)


def _source(engine, kind, reads, target, mode="HW", task="distance", k=-1, eqs=None):
    """a read batch of one of the three kinds a pair batch gathers from"""
    if kind == "both":
        return engine.BothStrandsBatch(reads, target, mode=mode, task=task, k=k, additionalEqualities=eqs)
    if kind == "hits":
        return engine.SharedBatch(reads, target, mode="HW", task="distance", k=max(k, 4), hits=True)
    return engine.SharedBatch(reads, target, mode=mode, task=task, k=k, additionalEqualities=eqs)


@pytest.fixture(scope="module")
def genome():
    """a 20,000-base ACGT target and 400 reads of 30 to 256 bases from both of its strands"""
    return PS.genome(2025, 12)


# ---- 1. source kinds x modes x tasks

@pytest.mark.parametrize("task", ["distance", "locations", "path"])
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
@pytest.mark.parametrize("kind", KINDS)
def test_set_shared_windows_equals_fresh_batch(engine, checker, genome, kind, mode, task):
    seed = KINDS.index(kind) * 100 + ["NW", "SHW", "HW"].index(mode) * 10 + ["distance", "locations", "path"].index(task)
    rng = np.random.default_rng(seed)
    k = 5 if seed % 2 else -1
    src = _source(engine, kind, genome["reads"], genome["target"])
    pb = engine.PairBatch([], [], mode=mode, task=task, k=k)
    try:
        if seed % 3 == 0:
            src.run()                                       # (a source that has run, and one that has not)
        tup = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), 1500, mode)
        assert tup.st.any() and not tup.st.all()
        got, stats = _set_and_compare(engine, checker, pb, src, genome["reads"], genome["target"], tup, mode, task, k,
                                      what=(kind, mode, task, k))
        assert stats["path"] & 2 and (got["editDistance"] >= 0).any()
        if k >= 0:
            assert (got["editDistance"] == -1).any()
    finally:
        pb.close()
        src.close()


# ---- 2. the shapes the gather can get wrong

# (a hit-list read batch takes targets of at most 16 symbols)
@pytest.mark.parametrize("kind,symbols", [(kind, s) for kind in KINDS for s in (4, 16, 40) if not (kind == "hits" and s > 16)])
def test_phase_length_alignment_grid(engine, checker, kind, symbols):
    """about 300 pairs over a 1,031-base target, every unit against the checker; targets of 4, 16 and 40 symbols (the last
    one SetWindows would refuse); reads of the lengths around the word and run sizes up to 1,024 bases -- those of 300
    and 1,024 long units of the source -- with IUPAC codes, lower case and U, on both strands from both pool layouts"""
    rng = np.random.default_rng(symbols + 1000 * KINDS.index(kind))
    A = np.arange(33, 33 + 5 * symbols, 5, dtype=np.uint8) if symbols > 4 else np.frombuffer(b"ACGT", dtype=np.uint8)
    assert len(A) == symbols and (symbols <= 16 or A.max() >= 128)
    Q = np.frombuffer(b"ACGTNacgtnUuRYKMBVDHSW", dtype=np.uint8)
    target = A[rng.integers(0, len(A), size=1031)].tobytes()
    lengths = QUERY_LENGTHS if kind != "hits" else QUERY_LENGTHS[:-2]
    reads = [Q[rng.integers(0, len(Q), size=m)].tobytes() for m in lengths]
    src = _source(engine, kind, reads, target)
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    short = engine.PairBatch([], [], mode="HW", task="path")
    try:
        tup = _grid(rng, len(target), len(reads))
        assert 280 <= len(tup) <= 320
        got, _ = _set_and_compare(engine, checker, pb, src, reads, target, tup, "HW", "locations", -1, everything=True,
                                  what=("grid", kind, symbols))
        assert got["alphabetLength"].max() >= symbols
        order = rng.permutation(len(tup))                # the same pairs in another order: every boundary elsewhere
        tup2 = Tuples(tup.q[order], tup.s[order], tup.n[order], tup.st[order])
        _set_and_compare(engine, checker, pb, src, reads, target, tup2, "HW", "locations", -1, everything=True,
                         what="permuted")
        # a NULL strand array is all forward
        _set_and_compare(engine, checker, pb, src, reads, target, Tuples(tup.q, tup.s, tup.n), "HW", "locations", -1,
                         everything=True, what="forward")
        # with paths: the reads a streamed HW set with paths takes (up to 256 bases)
        nshort = sum(m <= 256 for m in lengths)
        tup3 = Tuples(tup.q % nshort, tup.s, tup.n, tup.st)
        _set_and_compare(engine, checker, short, src, reads, target, tup3, "HW", "path", -1, everything=True, what="paths")
    finally:
        pb.close()
        short.close()
        src.close()


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025])
def test_counts(engine, checker, genome, n):
    rng = np.random.default_rng(300 + n)
    src = _source(engine, "both", genome["reads"], genome["target"])
    pb = engine.PairBatch([], [], mode="HW", task="locations")
    try:
        big = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), 1500, "HW")
        _set_and_compare(engine, checker, pb, src, genome["reads"], genome["target"], big, "HW", "locations", -1, what="before")
        tup = _mapper_tuples(rng, genome["reads"], genome["origin"], genome["strand"], len(genome["target"]), n, "HW")
        got, stats = _set_and_compare(engine, checker, pb, src, genome["reads"], genome["target"], tup, "HW", "locations", -1,
                                      everything=n < 1024, what=n)
        assert len(got["editDistance"]) == n and stats["path"] == (2 if n else 0), (n, stats)
    finally:
        pb.close()
        src.close()


# ---- 3. routes and states of the source

@pytest.mark.parametrize("kind", ["shared", "both"])
def test_a_source_above_the_inline_threshold(engine, checker, kind):
    """a 1,200,000-base target: the pools are buffers of their own, not views of the one uploaded block; windows at both
    of its ends; the source never Run, and the same source after a Run"""
    rng = np.random.default_rng(1200000)
    target = synth.random_dna(5, 1200000).tobytes()
    L = len(target)
    reads, origin, strand = _reads(rng, target, 64, 60, 200)
    src = _source(engine, kind, reads, target)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        for state in ("never run", "after a run"):
            tup = _mapper_tuples(rng, reads, origin, strand, L, 1100, "HW")
            tup.s[0], tup.n[0] = 0, 400
            tup.s[1], tup.n[1] = L - 400, 400
            tup.s[2], tup.n[2] = L - 1, 1
            tup.s[500], tup.n[500] = L - 65536, 65536
            _set_and_compare(engine, checker, pb, src, reads, target, tup, "HW", "path", -1, what=(kind, state))
            qs, ts = tup.materialise(reads, target)
            _check(pb, checker, qs, ts, "HW", "path", -1, sel=(0, 1, 2, 500), what=(kind, state))
            src.run()
    finally:
        pb.close()
        src.close()


def _source_views(src, kind):
    if kind == "hits":
        return dict(src.hits())
    out = dict(src.results_flat())
    if kind == "both":
        out["strand"], out["bothStrands"] = src.strands()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_the_source_is_left_as_it_was_and_may_go(engine, checker, genome, kind):
    rng = np.random.default_rng(401 + KINDS.index(kind))
    reads, target = genome["reads"], genome["target"]
    L = len(target)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    src = _source(engine, kind, reads, target, k=10)
    twin = _source(engine, kind, reads, target, k=10)      # never a source: what the source's own Run must still give
    try:
        tstats = twin.run()
        want = _source_views(twin, kind)

        def tuples():
            return _mapper_tuples(rng, reads, genome["origin"], genome["strand"], L, 1200, "HW")

        # before its first Run: the views still fail afterwards, and its first Run is the twin's
        _set_and_compare(engine, checker, pb, src, reads, target, tuples(), "HW", "path", -1, what=(kind, "no run yet"))
        with pytest.raises(RuntimeError):
            _source_views(src, kind)
        stats = src.run()
        _same(_source_views(src, kind), want, "the first run after a gather")
        assert {f: stats[f] for f in STATS} == {f: tstats[f] for f in STATS}
        # after a Run: the views held across the call, the views fetched afterwards, the next Run and its statistics
        held = src.hits(copy=False) if kind == "hits" else src.results_flat(copy=False)
        _set_and_compare(engine, checker, pb, src, reads, target, tuples(), "HW", "path", -1, what=(kind, "after a run"))
        _same(dict(held), {f: want[f] for f in held}, "views held across the gather")
        _same(_source_views(src, kind), want, "views after the gather")
        del held
        again = src.run()
        _same(_source_views(src, kind), want, "the next run")
        assert {f: again[f] for f in STATS} == {f: tstats[f] for f in STATS}

        # the bytes are copied: the source closes before the pair batch runs
        def gone():
            src.close()
            edlib_amd.lib().edlibAmdTrim()                 # its blocks go back to the driver

        tup = tuples()
        _set_and_compare(engine, checker, pb, src, reads, target, tup, "HW", "path", -1, what=(kind, "closed"), before_run=gone)
        want_pairs = _snapshot(pb)
        with pytest.raises(RuntimeError, match=NAME):
            pb.set_shared_windows(src, *tup.args())        # a closed batch is a NULL handle
        pb.run()
        _same(_snapshot(pb), want_pairs, "after the refusal")
    finally:
        pb.close()
        src.close()
        twin.close()


@pytest.mark.parametrize("mode,task", [("HW", "locations"), ("NW", "path")])
def test_the_pair_batch_keeps_its_own_equalities(engine, checker, mode, task):
    rng = np.random.default_rng(405)
    T = np.frombuffer(b"ACGTN", dtype=np.uint8)
    Q = np.frombuffer(b"ACGTRY", dtype=np.uint8)
    target = T[rng.integers(0, 5, size=20000)].tobytes()
    reads, origin, strand = _reads(rng, target, 300, 30, 200, sub=0.02)
    # (reads with codes the target does not hold: R and Y match by the pair batch's list alone)
    reads = [bytes(Q[rng.integers(0, 6)] if rng.random() < 0.05 else c for c in r) for r in reads]
    src = engine.SharedBatch(reads, target, mode="HW")     # no equalities
    pb = engine.PairBatch([], [], mode=mode, task=task, additionalEqualities=IUPAC)
    try:
        tup = _mapper_tuples(rng, reads, origin, strand, len(target), 1150, mode)
        _set_and_compare(engine, checker, pb, src, reads, target, tup, mode, task, -1, eqs=IUPAC, what=(mode, task))
    finally:
        pb.close()
        src.close()


def test_set_pairs_set_windows_and_set_shared_windows_on_one_batch(engine, checker, genome):
    rng = np.random.default_rng(404)
    reads, target = genome["reads"], genome["target"]
    n = len(reads)
    src = _source(engine, "shared", reads, target)
    wb = engine.WindowBatch(reads, target, np.arange(n), np.zeros(n), np.full(n, 300), mode="HW")
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        for c in range(2):
            tup = _mapper_tuples(rng, reads, genome["origin"], genome["strand"], len(target), 1100 + 100 * c, "HW")
            _set_and_compare(engine, checker, pb, src, reads, target, tup, "HW", "path", -1, what=("reads", c))
            before = _snapshot(pb)
            pb.set_windows(wb, *tup.args())                # the same tuples from the 4-bit pack: the same batch
            pb.run()
            _same(_snapshot(pb), before, ("windows", c))
            other = _mapper_tuples(rng, reads, genome["origin"], genome["strand"], len(target), 1300, "HW")
            qs, ts = other.materialise(reads, target)
            pb.set_pairs(qs, ts)
            pb.run()
            want, _ = _fresh(engine, qs, ts, "HW", "path", -1)
            _same(_snapshot(pb), want, ("pairs", c))
    finally:
        pb.close()
        wb.close()
        src.close()


# ---- 4. end to end: a distance Run, the first-hit windows, a path Run

def test_first_hits_of_a_both_strand_batch_get_the_whole_targets_path(engine, checker):
    rng = np.random.default_rng(77)
    target = synth.random_dna(21, 20000).tobytes()
    t = np.frombuffer(target, dtype=np.uint8)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = []
    for i in range(300):
        m = int(rng.integers(60, 251))
        if i % 15 == 7:
            q = A[rng.integers(0, 4, m)]                   # unrelated
        else:
            s = int(rng.integers(0, len(t) - m + 1))
            q = t[s:s + m].copy()
            hit = rng.random(m) < rng.random() * 0.10
            q[hit] = A[rng.integers(0, 4, int(hit.sum()))]
            if rng.random() < 0.4:
                p = int(rng.integers(1, m - 1))
                q = np.concatenate([q[:p], q[p + 1:]]) if rng.random() < 0.5 else np.concatenate([q[:p], A[:1], q[p:]])
        q = q.tobytes()
        reads.append(edlib_amd.reverse_complement(q) if i & 1 else q)
    src = engine.BothStrandsBatch(reads, target, mode="HW", task="distance", k=40)
    pb = engine.PairBatch([], [], mode="HW", task="path")
    try:
        src.run()
        flat = src.results_flat()
        strand, _ = src.strands()
        read, start, length, st = edlib_amd.first_hit_windows(flat, [len(r) for r in reads], strand)
        assert read.tolist() == np.flatnonzero(flat["editDistance"] >= 0).tolist()
        assert 250 <= len(read) < 300 and st.any() and not st.all()
        pb.set_shared_windows(src, read, start, length, st)
        src.close()
        pb.run()
        got = pb.results_flat()
        bad = []
        for i, r in enumerate(read):
            q = edlib_amd.reverse_complement(reads[r]) if st[i] else reads[r]
            want = checker.align(q, target, "HW", "path", -1)
            lo, ao = int(got["locOff"][i]), got["alnOff"]
            mine = (int(got["editDistance"][i]), int(got["ends"][lo]) + int(start[i]), int(got["starts"][lo]) + int(start[i]),
                    got["alignment"][int(ao[i]):int(ao[i + 1])].tobytes())
            theirs = (want["editDistance"], want["endLocations"][0], want["startLocations"][0], want["alignment"])
            if mine != theirs or mine[0] != flat["editDistance"][r]:
                bad.append((int(r), mine[:3], theirs[:3]))
        assert not bad, bad[:5]
    finally:
        pb.close()
        src.close()


# ---- 5. refusals leave the pair batch as it was

@pytest.mark.parametrize("mode", ["HW", "NW"])
def test_refusals_leave_the_pair_batch_as_it_was(engine, checker, mode):
    rng = np.random.default_rng(501)
    target = synth.random_dna(3, 70001).tobytes()
    L = len(target)
    reads, origin, strand = _reads(rng, target, 60, 60, 200)
    good = list(reads)
    reads[7] = b""                                        # (a read batch takes an empty read; a streamed pair set does not)
    reads[8] = b"ACGT" * 64                               # 256 bases
    reads[9] = target[100:400]                            # 300 bases: above a streamed SHW / HW set with paths
    reads[10] = target[1000:2025]                         # 1,025 bases: above any streamed set
    n = len(reads)
    src = engine.SharedBatch(reads, target, mode="HW")
    pb = engine.PairBatch([], [], mode=mode, task="path")
    lib = engine.lib()
    try:
        first = _mapper_tuples(rng, good, origin, strand, L, 1200, mode)
        first.q[(first.q >= 7) & (first.q <= 10)] = 11
        pb.set_shared_windows(src, *first.args())
        pb.run()
        before = _snapshot(pb)
        ok = Tuples([1, 2, 3, 4], [10, 20, 30, 40], [200, 210, 220, 230], [0, 1, 0, 1])

        def raw(source, q, s, ln, st, count):
            ptr = lambda a: None if a is None else a.ctypes.data
            return lib.edlibAmdBatchPairsSetSharedWindows(pb._h, None if source is None else source._h, ptr(q), ptr(s),
                                                          ptr(ln), ptr(st), count)

        def refused(call, *words):
            _refused(engine, pb, before, call, *words)

        def with_pair(at, q=None, s=None, ln=None, st=None):
            t = Tuples(ok.q.copy(), ok.s.copy(), ok.n.copy(), ok.st.copy())
            for arr, v in ((t.q, q), (t.s, s), (t.n, ln), (t.st, st)):
                if v is not None:
                    arr[at] = v
            return lambda: raw(src, t.q, t.s, t.n, t.st, len(t))

        refused(lambda: raw(None, ok.q, ok.s, ok.n, ok.st, 4), "null", "read batch")
        refused(lambda: raw(src, ok.q, ok.s, ok.n, ok.st, -1), "numPairs", "-1")
        refused(lambda: raw(src, None, ok.s, ok.n, ok.st, 4), "NULL")
        refused(lambda: raw(src, ok.q, None, ok.n, ok.st, 4), "NULL")
        refused(lambda: raw(src, ok.q, ok.s, None, None, 4), "NULL")
        refused(with_pair(2, q=n), "pair 2", "query %d" % n, "numQueries = %d" % n, "read batch")
        refused(with_pair(1, q=-1), "pair 1", "query -1")
        refused(with_pair(3, s=-5), "pair 3", "negative pairStart", "-5")
        refused(with_pair(0, ln=-2), "pair 0", "negative pairLength", "-2")
        refused(with_pair(2, s=L - 100, ln=101), "pair 2", "past the target", str(L - 100), "101", str(L))
        refused(with_pair(3, st=2), "pair 3", "pairStrand 2")
        refused(with_pair(1, q=7), "pair 1", "empty query", "create a new batch")
        refused(with_pair(2, ln=0), "pair 2", "empty target", "create a new batch")
        refused(with_pair(0, q=10), "pair 0", "1,025", "1,024", "create a new batch")
        refused(with_pair(3, s=4464, ln=65537), "pair 3", "65,537", "65,536", "create a new batch")
        if mode == "HW":
            refused(with_pair(1, q=9), "pair 1", "300", "256", "EDLIB_TASK_PATH", "HW", "create a new batch")
        else:
            # the linear-space regime: (20 blocks + 8) T >= 1 MiB
            refused(with_pair(1, q=8, s=0, ln=12000), "pair 1", "256", "12,000", "linear-space", "create a new batch")
        # the caps of a set with paths, decided on the host from the lengths alone (nothing is allocated for a refused set):
        # the column stores, 64 bytes per column and block row of every pair's window (HW: of 2 m + 1 columns), above 32 GB
        w = 513 if mode == "HW" else 11900                # (NW: 256 x 11,900 stays below the 1 MiB rule)
        at = 2 ** 35 // (64 * (w + 4))                    # the pair that passes the cap
        many = np.zeros(at + 3, dtype=np.int32)
        refused(lambda: raw(src, many + 8, many, many + (770 if mode == "HW" else w), None, len(many)),
                "pair %d" % at, "column stores", "32 GB", "EDLIB_TASK_PATH", "create a new batch")
        if mode == "HW":
            # ... and the op slots, m + window + 8 bytes a pair, above 8 GB: 256-base reads in one-column windows pass it
            # before their stores pass theirs -- 32.4 M tuples, the one heavy host pass of this file
            at = 2 ** 33 // (256 + 1 + 8)
            many = np.zeros(at + 3, dtype=np.int32)
            refused(lambda: raw(src, many + 8, many, many + 1, None, len(many)),
                    "pair %d" % at, "op slots", "8 GB", "EDLIB_TASK_PATH", "create a new batch")
        del many
        if engine.device_count() > 1:
            far = engine.SharedBatch(good[:2], target, mode="HW", device=1)
            try:
                assert raw(far, ok.q, ok.s, ok.n, ok.st, 4) != 0
                assert NAME in engine.last_error() and "device 1" in engine.last_error(), engine.last_error()
            finally:
                far.close()
        # a set that is taken still goes through
        _set_and_compare(engine, checker, pb, src, reads, target, first, mode, "path", -1, what="after the refusals")
    finally:
        pb.close()
        src.close()


def test_other_kinds_of_batch_are_refused_by_name(engine, genome):
    reads = [b"ACGTACGTAC", b"TTGACCA"]
    target = genome["target"][:400]
    z = np.zeros(2, dtype=np.int32)
    src = engine.SharedBatch(reads, target)
    pairs = engine.PairBatch(reads, [target, target], mode="HW", task="locations")
    lib = engine.lib()
    try:
        pairs.run()
        before = pairs.results_flat()
        as_pairs = [
            (lambda: engine.SharedBatch(reads, target), "a shared-target read batch"),
            (lambda: engine.BothStrandsBatch(reads, target), "a both-strand read batch"),
            (lambda: engine.CrossBatch(reads, [target]), "a cross batch"),
            (lambda: engine.SelfBatch(reads), "a self batch"),
            (lambda: engine.WindowBatch(reads, target, z, z, z + 50), "a window batch"),
        ]
        for make, kind in as_pairs:
            b = make()
            try:
                b.run()
                assert lib.edlibAmdBatchPairsSetSharedWindows(b._h, src._h, z.ctypes.data, z.ctypes.data,
                                                              (z + 50).ctypes.data, None, 2) != 0
                msg = engine.last_error()
                assert NAME in msg and kind in msg, msg
                b.run()                                   # the batch is what it was
            finally:
                b.close()
        assert lib.edlibAmdBatchPairsSetSharedWindows(None, src._h, z.ctypes.data, z.ctypes.data, (z + 50).ctypes.data,
                                                      None, 2) != 0
        assert NAME in engine.last_error() and "null pair batch" in engine.last_error(), engine.last_error()
        as_reads = [
            (lambda: engine.PairBatch(reads, [target, target]), "a pair batch"),
            (lambda: engine.PairBatch(reads[:1], [target]), "a pair batch"),          # (one pair: a shared target inside)
            (lambda: engine.CrossBatch(reads, [target]), "a cross batch"),
            (lambda: engine.CrossBatch(reads, [target], k=3, occurrences=True), "an occurrence batch"),
            (lambda: engine.SelfBatch(reads), "a self batch"),
            (lambda: engine.WindowBatch(reads, target, z, z, z + 50), "a window batch"),
        ]
        for make, kind in as_reads:
            b = make()
            try:
                assert lib.edlibAmdBatchPairsSetSharedWindows(pairs._h, b._h, z.ctypes.data, z.ctypes.data,
                                                              (z + 50).ctypes.data, None, 2) != 0
                msg = engine.last_error()
                assert NAME in msg and kind in msg and "read batch" in msg, msg
                pairs.run()
                _same(pairs.results_flat(), before, kind)
            finally:
                b.close()
    finally:
        pairs.close()
        src.close()
