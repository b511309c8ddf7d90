"""CPU model (numpy) of hit-list read batches (edlibAmdBatchCreateSharedHits).

D[j], j = 0 .. T-1, is the HW bottom-row score of a read against the target: the least edit distance between the read and
any substring of the target that ends at column j (the empty one counts, so D[j] <= m; there is no column -1 here).  A hit
is a maximal run [firstEnd, lastEnd] of consecutive columns with D[j] <= k; its editDistance is the least D of the run, its
endLocation the lowest column of the run holding that least value, its numLocations the number of columns holding it.

  * d_row() is the textbook DP of the bottom row (one row of the matrix at a time, vectors along the target);
  * d_rows() is Myers' bit-vector recurrence over 64-bit words for many reads at once (the GPU tests' batches: a row per
    read against 65,536 columns in seconds); tests/test_hits_model.py holds it against d_row();
  * hits() lists the hits of one row, hits_csr() those of many rows in the layout of EdlibAmdReadHits;
  * stitch() joins runs that meet end to end (segment boundaries), as the device's finish does."""
import numpy as np


def _equal_matrix(eq):
    """E[a, b]: bytes a and b are equal (identity plus the pairs of additionalEqualities, both ways)"""
    E = np.eye(256, dtype=bool)
    for a, b in (eq or ()):
        a = a[0] if isinstance(a, (bytes, bytearray)) else ord(a)
        b = b[0] if isinstance(b, (bytes, bytearray)) else ord(b)
        E[a, b] = E[b, a] = True
    return E


def _u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=np.uint8)


def d_row(read, target, eq=None):
    """D[0 .. T-1] by the textbook recurrence, row by row: D[i][j] = min(D[i-1][j-1] + (read[i] != target[j]),
    D[i-1][j] + 1, D[i][j-1] + 1), D[-1][j] = 0 (HW), D[i][-1] = i + 1"""
    q, t = _u8(read), _u8(target)
    T = len(t)
    E = _equal_matrix(eq)
    cols = np.arange(T, dtype=np.int64)
    prev = np.zeros(T, dtype=np.int64)                      # row -1
    for i in range(len(q)):
        diag = np.concatenate(([i], prev[:-1])) if T else prev
        tmp = np.minimum(diag + ~E[q[i], t], prev + 1)
        # horizontal moves: D[i][j] = min over j' <= j of tmp[j'] + (j - j'), and column -1 (value i + 1) before everything
        prev = np.minimum(np.minimum.accumulate(tmp - cols) + cols, i + 2 + cols)
    return prev


def d_rows(reads, target, eq=None):
    """D of every read (a list of byte strings / uint8 arrays of 1 .. 64 W bases) as an int32 array [reads, T], by Myers'
    recurrence on W 64-bit words per read.  `target`: one sequence for all reads, or a uint8 array [reads, T] with a row
    per read (columns past a row's own length hold anything: ignore them in the result)."""
    reads = [_u8(r) for r in reads]
    n = len(reads)
    t = np.asarray(target, dtype=np.uint8) if isinstance(target, np.ndarray) else _u8(target)
    own = t.ndim == 2
    T = t.shape[-1]
    out = np.zeros((n, T), dtype=np.int32)
    if n == 0 or T == 0:
        return out
    m = np.array([len(r) for r in reads], dtype=np.int64)
    assert m.min() >= 1
    W = int((m.max() + 63) // 64)
    E = _equal_matrix(eq)
    syms = np.unique(t)
    code = np.zeros(256, dtype=np.int64)
    code[syms] = np.arange(len(syms))
    # Peq[read, symbol, word]: bit r of word w = read[64 w + r] equals the symbol
    peq = np.zeros((n, len(syms), W), dtype=np.uint64)
    for i, r in enumerate(reads):
        bits = np.zeros((len(syms), 64 * W), dtype=bool)
        bits[:, :len(r)] = E[r][:, syms].T
        peq[i] = np.packbits(bits.reshape(len(syms), W, 64), axis=-1, bitorder="little").view(np.uint64).reshape(len(syms), W)
    one, top = np.uint64(1), np.uint64(63)
    Pv = np.full((W, n), ~np.uint64(0), dtype=np.uint64)
    Mv = np.zeros((W, n), dtype=np.uint64)
    lastw = (m - 1) // 64
    sh = ((m - 1) % 64).astype(np.uint64)
    score = m.copy()
    rows = np.arange(n)
    tc = code[t]
    for j in range(T):
        eqs = peq[rows, tc[:, j]] if own else peq[:, tc[j]]              # [n, W]
        hp = np.zeros(n, dtype=np.uint64)                                 # horizontal delta entering the word: +1 / -1 bits
        hn = np.zeros(n, dtype=np.uint64)
        for w in range(W):
            Eq = eqs[:, w]
            pv, mv = Pv[w], Mv[w]
            Xv = Eq | mv
            Eq = Eq | hn
            Xh = (((Eq & pv) + pv) ^ pv) | Eq
            Ph = mv | ~(Xh | pv)
            Mh = pv & Xh
            here = lastw == w
            if here.any():
                d = ((Ph >> sh) & one).astype(np.int64) - ((Mh >> sh) & one).astype(np.int64)
                score = score + np.where(here, d, 0)
            hp2, hn2 = Ph >> top, Mh >> top
            Ph = (Ph << one) | hp
            Mh = (Mh << one) | hn
            Pv[w] = Mh | ~(Xv | Ph)
            Mv[w] = Ph & Xv
            hp, hn = hp2, hn2
        out[:, j] = score
    return out


def hits(D, k):
    """the hits of one row: [(firstEnd, lastEnd, editDistance, endLocation, numLocations)], ascending"""
    D = np.asarray(D)
    out = []
    j, T = 0, len(D)
    while j < T:
        if D[j] > k:
            j += 1
            continue
        a = j
        while j < T and D[j] <= k:
            j += 1
        run = D[a:j]
        lo = int(run.min())
        out.append((a, j - 1, lo, a + int(np.argmax(run == lo)), int(np.count_nonzero(run == lo))))
    return out


def hits_csr(rows, k, lengths=None):
    """the hits of many rows (int array [reads, T]; lengths: columns that count per row, default all) as the arrays of
    EdlibAmdReadHits: unitOffsets int64 [reads + 1], firstEnd / lastEnd / editDistance / endLocation / numLocations int32"""
    rows = np.asarray(rows)
    n, T = rows.shape
    within = rows <= k
    if lengths is not None:
        within &= np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    pad = np.zeros((n, T + 2), dtype=np.int8)
    pad[:, 1:-1] = within
    edge = np.diff(pad, axis=1)                                           # +1 at a run's first column, -1 behind its last
    r0, first = np.nonzero(edge == 1)
    _, last = np.nonzero(edge == -1)
    last = last - 1
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r0, minlength=n), out=off[1:])
    names = ("firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations")
    if len(first) == 0:
        return dict({f: np.zeros(0, dtype=np.int32) for f in names}, unitOffsets=off, numHits=0)
    # the least score and its first column from one reduction over (score << 32 | column); runs in row-major order
    flat = ((rows.astype(np.int64) << 32) | np.arange(T, dtype=np.int64)[None, :]).reshape(-1)
    flat = np.where(within.reshape(-1), flat, np.int64(1) << 62)
    starts = r0 * T + first
    key = np.minimum.reduceat(flat, starts)                               # (a run ends where a column outside follows)
    ed, end = key >> 32, key & 0xffffffff
    run_of = np.cumsum(np.bincount(starts, minlength=n * T)) - 1                     # the last run that started at or before a cell
    same = within.reshape(-1) & (rows.reshape(-1) == ed[np.maximum(run_of, 0)])
    cnt = np.add.reduceat(same.astype(np.int64), starts)
    # (reduceat sums up to the next run's start: columns between two runs are outside `within`, hence not counted)
    vals = (first, last, ed, end, cnt)
    return dict({f: v.astype(np.int32) for f, v in zip(names, vals)}, unitOffsets=off, numHits=len(first))


def stitch(runs):
    """runs (firstEnd, lastEnd, editDistance, endLocation, numLocations) sorted by firstEnd; two that meet (lastEnd + 1 ==
    the next firstEnd) become one: the least distance, the first column holding it, the counts of the parts attaining it"""
    out = []
    for f, l, ed, pos, cnt in runs:
        if out and out[-1][1] + 1 == f:
            pf, _, ped, ppos, pcnt = out[-1]
            if ed < ped:
                out[-1] = (pf, l, ed, pos, cnt)
            elif ed == ped:
                out[-1] = (pf, l, ped, ppos, pcnt + cnt)
            else:
                out[-1] = (pf, l, ped, ppos, pcnt)
        else:
            out.append((f, l, ed, pos, cnt))
    return out
