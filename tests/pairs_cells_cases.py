"""What the tests of pairs gathered from a cross or self batch share (test_gpu_pairs_cells.py: set_cells;
edlibAmdBatchPairsSetCells): the (query, target, window, strand) tuples with their materialisation over a LIST of
targets, the nine kinds of source and what a caller can read of each, and sets of related queries and targets.  The
yardstick itself is tests/pairs_set_cases.py (snapshot, same, fresh, check, refused, set_and_compare), used as it is: a
CellTuples goes where it takes a Tuples, the list of targets where it takes the target.  A plain module, not a conftest."""
import numpy as np

import edlib_amd

CROSS_KINDS = ("cross", "hits", "occ", "both", "hitsboth")
SELF_KINDS = ("self", "selfhits", "selfboth", "selfhitsboth")
KINDS = CROSS_KINDS + SELF_KINDS
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


class CellTuples:
    """(query, target, start, length, strand) per pair, as set_cells takes them; s and n None: whole targets"""

    def __init__(self, q, t, s=None, n=None, st=None):
        self.q, self.t = (np.asarray(a, dtype=np.int32) for a in (q, t))
        self.s = None if s is None else np.asarray(s, dtype=np.int32)
        self.n = None if n is None else np.asarray(n, dtype=np.int32)
        self.st = None if st is None else np.asarray(st, dtype=np.uint8)

    def __len__(self):
        return len(self.q)

    def args(self):
        return self.q, self.t, self.s, self.n, self.st

    def take(self, idx):
        pick = lambda a: None if a is None else a[idx]
        return CellTuples(self.q[idx], self.t[idx], pick(self.s), pick(self.n), pick(self.st))

    def materialise(self, queries, targets):
        """the pairs on the host: slices of the targets, reverse complements of the queries of strand 1"""
        return materialise(queries, targets, *self.args())


def materialise(queries, targets, q, t, s=None, n=None, st=None):
    qs = [bytes(queries[a]) if (st is None or not st[i]) else edlib_amd.reverse_complement(bytes(queries[a]))
          for i, a in enumerate(q)]
    if s is None:
        return qs, [bytes(targets[b]) for b in t]
    return qs, [bytes(targets[b])[int(lo):int(lo) + int(ln)] for b, lo, ln in zip(t, s, n)]


def source(engine, kind, queries, targets=None, mode="HW", k=10, eqs=None):
    """a batch of one of the nine kinds a pair batch gathers cells from (a self kind: `queries` is the one set, NW)"""
    if kind in SELF_KINDS:
        return engine.SelfBatch(queries, k=k if "hits" in kind else -1, additionalEqualities=eqs, hits="hits" in kind,
                                strands="both" if "both" in kind else "forward")
    if kind == "occ":
        return engine.CrossBatch(queries, targets, mode="HW", k=k, additionalEqualities=eqs, occurrences=True)
    return engine.CrossBatch(queries, targets, mode=mode, k=k if "hits" in kind else -1, additionalEqualities=eqs,
                             hits="hits" in kind, strands="both" if "both" in kind else "forward")


def source_views(src, kind, copy=True):
    """everything a caller can read of a source after a Run (copy=False: views of the batch's own memory)"""
    if kind == "occ":
        return dict(src.occurrences(copy=copy))
    if kind in SELF_KINDS:
        out = dict(src.hits(copy=copy)) if "hits" in kind else {"condensed": src.condensed(copy=copy)}
        out.update(src.nearest(copy=copy))
    else:
        out = dict(src.hits(copy=copy)) if "hits" in kind else dict(src.matrix(copy=copy))
        out.update(src.best(copy=copy))
    if "both" in kind:
        out.update(src.strands(copy=copy))
    return out


def related(rng, num_queries, num_targets, qlo=20, qhi=256, tlo=1, thi=2000, sub=0.03):
    """targets of tlo..thi random bases in no order of length, some lengths repeated, and queries cut from them with a few
    substitutions and now and then an indel, every other one from the reverse strand; where each query came from"""
    lens = rng.integers(tlo, thi + 1, size=num_targets)
    lens[1::7] = lens[0]                                   # repeated lengths
    lens[3] = max(thi, qhi)
    targets = [DNA[rng.integers(0, 4, size=int(n))].tobytes() for n in lens]
    queries, origin_t, origin_s, strand = [], [], [], []
    for i, m in enumerate(rng.integers(qlo, qhi + 1, size=num_queries)):
        m = int(m)
        t = int(rng.choice(np.flatnonzero(lens >= m)))
        s = int(rng.integers(0, lens[t] - m + 1))
        q = np.frombuffer(targets[t], dtype=np.uint8)[s:s + m].copy()
        at = rng.integers(0, m, size=rng.binomial(m, sub))
        q[at] = DNA[rng.integers(0, 4, size=len(at))]
        if m > 4 and rng.random() < 0.3:
            p = int(rng.integers(1, m - 1))
            q = np.concatenate([q[:p], q[p + 1:], DNA[rng.integers(0, 4, size=1)]])
        st = i & 1
        queries.append(edlib_amd.reverse_complement(q.tobytes()) if st else q.tobytes())
        origin_t.append(t); origin_s.append(s); strand.append(st)
    return {"queries": queries, "targets": targets, "origin_t": np.array(origin_t), "origin_s": np.array(origin_s),
            "strand": np.array(strand)}


def cell_tuples(rng, data, n, mode):
    """n pairs in no order: mostly a query in its strand against a window around where it came from (NW: about its span,
    SHW: from its first column on, HW: padded on both sides), the others against any window of any target, either strand"""
    queries, targets = data["queries"], data["targets"]
    tl = np.array([len(t) for t in targets], dtype=np.int64)
    q = rng.integers(0, len(queries), size=n)
    m = np.array([len(queries[i]) for i in q], dtype=np.int64)
    # (queries without a known origin -- none has one where origin_t is empty -- take any window)
    known = q < len(data["origin_t"])
    home = (rng.random(n) < 0.7) & known
    oq = np.where(known, q, 0)
    pad = lambda a: np.concatenate([np.asarray(a, dtype=np.int64), np.zeros(len(queries), dtype=np.int64)])
    origin_t, origin_s, strand = pad(data["origin_t"]), pad(data["origin_s"]), pad(data["strand"])
    t = np.where(home, origin_t[oq], rng.integers(0, len(targets), size=n))
    t[tl[t] == 0] = int(np.argmax(tl))
    T = tl[t]
    st = np.where(home & (rng.random(n) < 0.9), strand[oq], rng.integers(0, 2, size=n))
    if mode == "NW":
        lead, trail = rng.integers(0, 3, size=n), rng.integers(0, 3, size=n)
    elif mode == "SHW":
        lead, trail = np.zeros(n, dtype=np.int64), rng.integers(0, 2 * m + 1)
    else:
        lead, trail = rng.integers(0, m + 1), rng.integers(0, m + 1)
    s = np.maximum(origin_s[oq] - lead, 0)
    e = np.minimum(origin_s[oq] + m + trail, T)
    rs = (rng.random(n) * T).astype(np.int64)              # any window of any target
    re = rs + 1 + (rng.random(n) * (T - rs)).astype(np.int64)
    s, e = np.where(home, s, rs), np.where(home, e, np.minimum(re, T))
    return CellTuples(q, t, s, e - s, st)
