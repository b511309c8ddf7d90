"""CPU model (numpy) of occurrence cross batches (edlibAmdBatchCreateCrossOccurrences, DESIGN.md §4h "Occurrence batches"),
built on hits_model: the definition of a hit-list read batch per (query, target) cell, with target-relative columns.

occurrences() gives the arrays of EdlibAmdCrossOccurrences for a case: grouped by target in the caller's order (CSR), inside
a target by ascending query, inside a cell by ascending firstEnd.  An empty query occurs once in every non-empty target
([0, n-1], distance 0, endLocation 0, numLocations n); an empty target holds no occurrence."""
import numpy as np

import hits_model as H

FIELDS = ("query", "firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations")
RUN = ("firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations")


def occurrences(queries, targets, k, eq=None):
    queries = [bytes(q) for q in queries]
    targets = [bytes(t) for t in targets]
    nq, nt = len(queries), len(targets)
    tl = np.array([len(t) for t in targets], dtype=np.int64)
    live = [q for q in range(nq) if len(queries[q]) > 0]
    tmax = int(tl.max()) if nt else 0
    csr = None
    if live and tmax > 0:
        # a row per (target, query) cell against its own target (d_rows with a 2-D target), target-major
        tm = np.zeros((nt, tmax), dtype=np.uint8)
        for t, s in enumerate(targets):
            tm[t, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        rows = H.d_rows([queries[q] for _ in range(nt) for q in live], np.repeat(tm, len(live), axis=0), eq)
        csr = H.hits_csr(rows, k, np.repeat(tl, len(live)))
    cols = {f: [] for f in FIELDS}
    off = np.zeros(nt + 1, dtype=np.int64)
    for t in range(nt):
        n = int(tl[t])
        li = 0
        for q in range(nq):
            if len(queries[q]) == 0:
                if n > 0:
                    for f, v in zip(FIELDS, (q, 0, n - 1, 0, 0, n)):
                        cols[f].append(np.array([v], dtype=np.int32))
                continue
            r = t * len(live) + li
            li += 1
            a, b = (int(csr["unitOffsets"][r]), int(csr["unitOffsets"][r + 1])) if csr is not None else (0, 0)
            if b > a:
                cols["query"].append(np.full(b - a, q, dtype=np.int32))
                for f in RUN:
                    cols[f].append(csr[f][a:b])
        off[t + 1] = sum(len(x) for x in cols["query"])
    out = {f: (np.concatenate(v).astype(np.int32) if v else np.zeros(0, dtype=np.int32)) for f, v in cols.items()}
    out["targetOffsets"] = off
    return out


def cell_runs(occ, t, q):
    """[(firstEnd, lastEnd, editDistance, endLocation, numLocations)] of cell (t, q) of an occurrences() / view dictionary"""
    a, b = int(occ["targetOffsets"][t]), int(occ["targetOffsets"][t + 1])
    return [tuple(int(occ[f][i]) for f in RUN) for i in range(a, b) if int(occ["query"][i]) == q]


def assert_equal(got, want):
    """the whole view, field by field"""
    assert np.array_equal(np.asarray(got["targetOffsets"]), want["targetOffsets"]), \
        (np.asarray(got["targetOffsets"])[:8], want["targetOffsets"][:8])
    for f in FIELDS:
        g = np.asarray(got[f])
        assert g.shape == want[f].shape, (f, g.shape, want[f].shape)
        bad = np.nonzero(g != want[f])[0]
        assert len(bad) == 0, (f, bad[:5], g[bad[:5]], want[f][bad[:5]])


def assert_ordered(occ, numQueries):
    """per target the queries ascend; inside a cell firstEnd ascends and runs are maximal (a gap of a column or more)"""
    off = np.asarray(occ["targetOffsets"])
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(occ["query"])
    for t in range(len(off) - 1):
        a, b = int(off[t]), int(off[t + 1])
        q = np.asarray(occ["query"][a:b]).astype(np.int64)
        assert np.all((q >= 0) & (q < numQueries))
        assert np.all(np.diff(q) >= 0), t
        same = np.diff(q) == 0
        first, last = np.asarray(occ["firstEnd"][a:b]).astype(np.int64), np.asarray(occ["lastEnd"][a:b]).astype(np.int64)
        assert np.all(first <= last)
        assert np.all(last[:-1][same] + 1 < first[1:][same]), t
