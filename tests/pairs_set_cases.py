"""What the GPU tests of the three ways to give a resident pair batch another set share (test_gpu_pairs_stream.py:
set_pairs, test_gpu_pairs_windows.py: set_windows, test_gpu_pairs_shared.py: set_shared_windows): the yardstick -- after
the set and a run() the batch is exactly a fresh PairBatch over the same pairs, and its units equal the checker -- and,
for the two calls that gather, the (query, strand, window) tuples a mapper would send.  A plain module, not a conftest:
the `engine` and `checker` fixtures are passed in by the tests."""
import numpy as np

import edlib_amd
from edlib_amd import synth

STATS = ("cells", "word_steps", "path", "scan_launches")
FIELDS = ("status", "editDistance", "endLocations", "startLocations", "numLocations", "alignment", "alignmentLength",
          "alphabetLength")
IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]
WINDOW_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 400)


# ---- the yardstick

def snapshot(b):
    """everything a caller can read after a run: results_flat() and both CIGAR forms"""
    out = dict(b.results_flat())
    for ext in (True, False):
        chars, off = b.cigars(extended=ext)
        out["cigar%d.chars" % ext], out["cigar%d.off" % ext] = chars, off
    return out


def same(got, want, what="", scalars=False):
    """two dicts of arrays (or None) are equal, shapes and dtypes included; scalars: entries that are no arrays may occur
    and compare by =="""
    assert sorted(got) == sorted(want), what
    for f in want:
        if want[f] is None or got[f] is None:
            assert got[f] is None and want[f] is None, (what, f)
            continue
        if scalars and not isinstance(want[f], np.ndarray):
            assert got[f] == want[f], (what, f)
            continue
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())


def fresh(engine, qs, ts, mode, task, k, eqs=None):
    b = engine.PairBatch(qs, ts, mode=mode, task=task, k=k, additionalEqualities=eqs)
    try:
        stats = b.run()
        return snapshot(b), stats
    finally:
        b.close()


def check(b, checker, qs, ts, mode, task, k, eqs=None, sel=None, what=""):
    """results() of the units `sel` (all: None) against the checker, every field"""
    got = b.results(raw=True)
    assert len(got) == len(qs)
    bad = []
    for i in (range(len(qs)) if sel is None else sel):
        want = checker.align(qs[i], ts[i], mode, task, k, eq_pairs=eqs)
        if any(got[i][f] != want[f] for f in FIELDS):
            bad.append((i, len(qs[i]), len(ts[i]), {f: (got[i][f], want[f]) for f in FIELDS if got[i][f] != want[f]}))
    assert not bad, (what, mode, task, k, bad[:3])


def refused(name, engine, pb, before, call, *words):
    """the call fails with a message that names the function `name` and carries `words`; the views held across it, the
    views fetched after it and the next Run are those of `before`"""
    held = pb.results_flat(copy=False)                    # views of the batch's own memory, held across the refusal
    cig = pb.cigars(copy=False)
    assert call() != 0
    msg = engine.last_error()
    assert name in msg and all(w in msg for w in words), msg
    for f, v in held.items():
        assert v is None or np.array_equal(v, before[f]), (msg, f)
    assert np.array_equal(cig[0], before["cigar1.chars"]) and np.array_equal(cig[1], before["cigar1.off"]), msg
    same(snapshot(pb), before, msg)
    del held, cig
    pb.run()                                              # ... and the next Run reproduces them
    same(snapshot(pb), before, ("the next run", msg))


# ---- sets gathered from another batch

class Tuples:
    """(query, start, length, strand) per pair, as set_windows and set_shared_windows take them"""

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


def reads(rng, target, count, lo=30, hi=256, sub=0.03):
    """reads cut from the target with a few substitutions and now and then an indel, every other one from the reverse
    strand; where each came from"""
    t = np.frombuffer(bytes(target), dtype=np.uint8)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    out, origin, strand = [], [], []
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
        out.append(edlib_amd.reverse_complement(q.tobytes()) if st else q.tobytes())
        origin.append(s)
        strand.append(st)
    return out, np.array(origin), np.array(strand)


def genome(seed, target_seed):
    """a 20,000-base ACGT target and 400 reads of 30 to 256 bases from both of its strands"""
    rng = np.random.default_rng(seed)
    target = synth.random_dna(target_seed, 20000).tobytes()
    rs, origin, strand = reads(rng, target, 400)
    return {"target": target, "reads": rs, "origin": origin, "strand": strand}


def mapper_tuples(rng, reads, origin, strand, target_length, n, mode):
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


def grid(rng, target_length, num_queries, phases, reps=1):
    """`reps` times every phase of a window's first column (modulo `phases`) x every window length, consecutive odd lengths
    (every alignment of the next pair), windows at column 0 and up to the last column, both strands"""
    ps, pl = [], []
    for rep in range(reps):
        for phase in range(phases):
            for n in WINDOW_LENGTHS:
                ps.append(phases * int(rng.integers(0, (target_length - 400) // phases - 1)) + phase)
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


def set_and_compare(setter, engine, checker, pb, src, queries, target, tup, mode, task, k, eqs=None, everything=False,
                    what="", before_run=None):
    """pb.<setter>(src, tuples) + run on pb against a fresh batch over the materialised pairs, and about 100 units (or all)
    against the checker; before_run() is called between the two (the source may go there)"""
    getattr(pb, setter)(src, *tup.args())
    assert pb.n == len(tup)
    if before_run is not None:
        before_run()
    stats = pb.run()
    got = snapshot(pb)
    qs, ts = tup.materialise(queries, target)
    want, wstats = fresh(engine, qs, ts, mode, task, k, eqs)
    same(got, want, what)
    # (a fresh batch of fewer than 1,024 pairs takes the general path, whose word_steps and launches are another count:
    # there the statistics are those of the batch set_pairs makes)
    if len(tup) < 1024:
        other = engine.PairBatch([], [], mode=mode, task=task, k=k, additionalEqualities=eqs)
        try:
            other.set_pairs(qs, ts)
            wstats = other.run()
            same(got, snapshot(other), ("set_pairs", what))
        finally:
            other.close()
    assert {f: stats[f] for f in STATS} == {f: wstats[f] for f in STATS}, what
    assert stats["cells"] == sum(len(q) * len(t) for q, t in zip(qs, ts)), what
    n = len(qs)
    check(pb, checker, qs, ts, mode, task, k, eqs, None if everything else range(0, n, max(1, n // 100)), what)
    return got, stats
