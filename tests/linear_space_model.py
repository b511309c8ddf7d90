"""A plain model of the linear-space NW path (the reference's obtainAlignment / obtainAlignmentHirschberg,
edlib.cpp:1161-1396) in our own words: the 1 MiB rule, textbook last columns in int64 numpy, the split rule with its
preference among equal sums, the recursion down to leaves that are below the rule, and a census of which branches an
input takes.  Leaves come from a callable (the C99 oracle or the compiled reference at NW / path), which is below the
rule and therefore restated by both.  Nothing here is imported from the product."""
import numpy as np

OP_MATCH, OP_INSERT, OP_DELETE, OP_MISMATCH = 0, 1, 2, 3
OP_CHARS = "=IDX"


def needs_rule(m, T):
    """The reference walks a stored matrix while (2 * 8 + 4) bytes per block and column plus 8 bytes per column stay
    below 1 MiB, and divides the problem otherwise (edlib.cpp:1188-1190)."""
    blocks = -(-m // 64)
    return (20 * blocks + 8) * T >= 1 << 20


def first_T(m):
    """The smallest T at which (m, T) meets the rule."""
    per_column = 20 * -(-m // 64) + 8
    return -(-(1 << 20) // per_column)


def equality_table(eq_pairs=None):
    """eq[a, b]: byte a of the query equals byte b of the target (identity plus the symmetric additional equalities)."""
    eq = np.eye(256, dtype=bool)
    for a, b in eq_pairs or ():
        a = a if isinstance(a, bytes) else a.encode("latin-1")
        b = b if isinstance(b, bytes) else b.encode("latin-1")
        eq[a[0], b[0]] = eq[b[0], a[0]] = True
    return eq


def last_column(q, t, eq=None):
    """D[0..m][T] of the textbook NW matrix (unit costs), one column at a time."""
    if eq is None:
        eq = equality_table()
    qa = np.frombuffer(bytes(q), dtype=np.uint8)
    m = len(qa)
    idx = np.arange(m + 1, dtype=np.int64)
    col = idx.copy()
    tmp = np.empty(m + 1, dtype=np.int64)
    t = bytes(t)
    cost = {c: (~eq[qa, c]).astype(np.int64) for c in set(t)}      # 1 where the query symbol differs from c
    for c in t:
        tmp[0] = col[0] + 1
        if m:
            np.minimum(col[:-1] + cost[c], col[1:] + 1, out=tmp[1:])
        # D[i] = min(tmp[i], D[i-1] + 1)  <=>  D[i] - i = min over i' <= i of (tmp[i'] - i')
        col = np.minimum.accumulate(tmp - idx) + idx
    return col


def split(q, t, score, eq=None):
    """(i, left score, right score, number of interior rows that attain the score): the row i of the query after which
    the path leaves the left half of the target.  First interior row 0..m-2, else -1 (the whole query goes right), else
    m-1 (the whole query goes left); None when no sum attains the score."""
    m, T = len(q), len(t)
    lw = T // 2
    rw = T - lw
    L = last_column(q, t[:lw], eq)                         # L[h]: q[:h] against the left half
    R = last_column(q[::-1], t[lw:][::-1], eq)[::-1]       # R[h]: q[h:] against the right half
    sums = L + R
    interior = np.flatnonzero(sums[1:m] == score) + 1 if m >= 2 else np.zeros(0, dtype=np.int64)
    if len(interior):
        h = int(interior[0])
        return h - 1, int(L[h]), int(R[h]), len(interior)
    if lw + int(R[0]) == score:
        return -1, lw, int(R[0]), 0
    if int(L[m]) + rw == score:
        return m - 1, int(L[m]), rw, 0
    return None


def new_census():
    return {"interior": 0, "interior_tie": 0, "top": 0, "bottom": 0, "empty_query_piece": 0, "depth": 0}


def path(q, t, score, leaf, eq_pairs=None):
    """(ops, census) of the NW path of (q, t) whose distance is `score`.  leaf(q, t, k) -> op bytes of a piece below the
    rule."""
    eq = equality_table(eq_pairs)
    census = new_census()
    out = bytearray()

    def piece(q, t, score, depth):
        m, T = len(q), len(t)
        if m == 0 or T == 0:
            if m == 0 and depth:
                census["empty_query_piece"] += 1
            out.extend(bytes([OP_DELETE if m == 0 else OP_INSERT]) * (m + T))
            return
        if not needs_rule(m, T):
            out.extend(leaf(q, t, score))
            return
        census["depth"] = max(census["depth"], depth + 1)
        found = split(q, t, score, eq)
        assert found is not None, ("no row attains the score", m, T, score)
        i, left, right, attaining = found
        if attaining:
            census["interior"] += 1
            census["interior_tie"] += attaining > 1
        elif i == -1:
            census["top"] += 1
        else:
            census["bottom"] += 1
        lw = T // 2
        piece(q[:i + 1], t[:lw], left, depth + 1)
        piece(q[i + 1:], t[lw:], right, depth + 1)

    piece(bytes(q), bytes(t), score, 0)
    return bytes(out), census


def leaf_of(impl, eq_pairs=None):
    """A leaf solver over a checker (`align(query, target, mode, task, k, eq_pairs)`)."""
    def leaf(q, t, k):
        assert not needs_rule(len(q), len(t))
        r = impl.align(q, t, "NW", "path", k, eq_pairs)
        assert r["status"] == 0 and r["editDistance"] == k, (len(q), len(t), k, r["status"], r["editDistance"])
        return r["alignment"]
    return leaf


def ops_to_cigar(ops):
    """Extended CIGAR of an op string."""
    a = np.frombuffer(bytes(ops), dtype=np.uint8)
    if len(a) == 0:
        return ""
    cut = np.flatnonzero(np.diff(a)) + 1
    starts = np.concatenate(([0], cut))
    lens = np.diff(np.concatenate((starts, [len(a)])))
    return "".join("%d%s" % (n, OP_CHARS[a[s]]) for s, n in zip(starts, lens))


def cigar_to_ops(cigar):
    """The op string of an extended CIGAR."""
    out = bytearray()
    n = 0
    for ch in cigar:
        if ch.isdigit():
            n = 10 * n + ord(ch) - 48
        else:
            out.extend(bytes([OP_CHARS.index(ch)]) * n)
            n = 0
    return bytes(out)


def assert_path_valid(q, t, ops, ed, eq_pairs=None):
    """The ops consume exactly the query and the target, '=' stands only on equal symbols, 'X' only on unequal ones, and
    the ops that are not '=' number `ed`."""
    eq = equality_table(eq_pairs)
    a = np.frombuffer(bytes(ops), dtype=np.uint8)
    qa = np.frombuffer(bytes(q), dtype=np.uint8)
    ta = np.frombuffer(bytes(t), dtype=np.uint8)
    assert a.size == 0 or a.max() <= 3
    takes_q = a != OP_DELETE
    takes_t = a != OP_INSERT
    assert int(takes_q.sum()) == len(qa), (int(takes_q.sum()), len(qa))
    assert int(takes_t.sum()) == len(ta), (int(takes_t.sum()), len(ta))
    qi = np.cumsum(takes_q) - 1                             # the query symbol an op consumes, where it consumes one
    ti = np.cumsum(takes_t) - 1
    diag = np.flatnonzero((a == OP_MATCH) | (a == OP_MISMATCH))
    same = eq[qa[qi[diag]], ta[ti[diag]]]
    is_match = a[diag] == OP_MATCH
    bad = np.flatnonzero(same != is_match)
    assert bad.size == 0, ("op disagrees with the symbols at op index", int(diag[bad[0]]))
    assert int((a != OP_MATCH).sum()) == ed, (int((a != OP_MATCH).sum()), ed)
