"""CPU model (numpy) of the exact k-mer seed filter that is the first pass of HW read groups against a target of at most
four symbols (edlib_amd/csrc/reads_seed.hip), used by tests/test_seed_model.py to check the ARGUMENT of that
path against the textbook DP without a GPU:

  * seed_threshold() is the host's k_f (Batch::seedThreshold);
  * pieces() cuts a read into k + 1 consecutive pieces of floor(m / (k + 1)) symbols or one more;
  * lookup() finds every exact occurrence of every piece through buckets on its first q symbols (pieces holding a byte the
    target lacks cannot occur and are skipped), giving the diagonals delta = P - o;
  * windows() merges [delta - k, delta + m - 1 + k] (clipped to the target) over the sorted, distinct diagonals;
  * predict() is what the kernel must DO for a read: whether it hands it back, how many distinct diagonals it finds and how
    many columns its merged windows hold (the kernel's work counter adds NWD word-steps per such column);
  * seed_filter() scans every window restarted from a fresh column (filter_model.bottom_row over the window) and returns the
    least score with the columns attaining it when that is <= k, None (unresolved) otherwise, or "back" when one of the caps
    of the kernel hands the read back to the banded scan."""
import numpy as np

from filter_model import bottom_row

Q = 12                      # kSeedQ
BUCKET_CAP = 64             # kSeedBucketCap
MAX_DIAG = 32               # kSeedMaxDiag
MAX_WINDOW = 1024           # kSeedMaxWindow


def seed_threshold(m_min, T, q=Q, kmax=16):
    """the largest k <= kmax whose pieces hold >= q symbols and whose expected random hits per read, (k + 1) T / 4^L,
    stay <= 1/8; -1 if there is none"""
    for k in range(kmax, -1, -1):
        L = m_min // (k + 1)
        if L >= q and (k + 1) * T * 8 <= 4 ** L:
            return k
    return -1


def pieces(m, k):
    """[(query offset, length)] of the k + 1 pieces"""
    p = k + 1
    L, r = divmod(m, p)
    return [(i * L + min(i, r), L + (1 if i < r else 0)) for i in range(p)]


def build_index(t, q):
    """bucket of the first q symbols -> target positions"""
    t = _bytes(t)
    idx = {}
    for P in range(len(t) - q + 1):
        idx.setdefault(t[P:P + q], []).append(P)
    return idx


def _bytes(x):
    return x if isinstance(x, bytes) else bytes(np.asarray(x, dtype=np.uint8))


def lookup(qr, t, k, q=Q, index=None, caps=True, present=None, info=None):
    """sorted distinct diagonals of the exact piece hits, or "back".  `t` may be the target's bytes and `present` the set
    of its byte values (a caller with many reads converts the target once); `info`, a dict, receives the largest bucket
    that was looked at"""
    qb = _bytes(qr); tb = _bytes(t)
    present = set(tb) if present is None else present
    index = build_index(tb, q) if index is None else index
    diags = set()
    for o, n in pieces(len(qb), k):
        if n < q:
            return "back"
        piece = qb[o:o + n]
        if any(c not in present for c in piece):        # a byte the target lacks: the piece cannot occur
            continue
        bucket = index.get(piece[:q], ())
        if info is not None:
            info["bucket"] = max(info.get("bucket", 0), len(bucket))
        if caps and len(bucket) > BUCKET_CAP:
            return "back"
        for P in bucket:
            if tb[P:P + n] == piece:
                diags.add(P - o)
                if caps and len(diags) > MAX_DIAG:
                    return "back"
    return sorted(diags)


def windows(diags, m, k, T):
    """merged [a, b] windows of the sorted diagonals"""
    out = []
    for d in diags:
        a, b = max(0, d - k), min(T - 1, d + m - 1 + k)
        if out and a <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(w) for w in out]


def predict(read, target, k, index, present=None, q=Q):
    """what the kernel does with one read at threshold k, caps on: {"back": handed back, "diagonals": distinct diagonals,
    "columns": sum of the merged window lengths, "bucket": the largest bucket looked at, "window": the longest merged
    window}; a handed-back read verifies no column.  `target` as bytes, `index` = build_index(target, q) and `present` =
    set(target) make a batch of thousands of reads cost seconds."""
    tb = _bytes(target)
    info = {}
    diags = lookup(read, tb, k, q, index, True, present, info)
    out = {"back": True, "diagonals": 0, "columns": 0, "bucket": info.get("bucket", 0), "window": 0}
    if diags == "back":
        return out
    ws = windows(diags, len(read), k, len(tb))
    out["window"] = max([b - a + 1 for a, b in ws], default=0)
    if out["window"] > MAX_WINDOW:
        return out
    out.update(back=False, diagonals=len(diags), columns=sum(b - a + 1 for a, b in ws))
    return out


def predict_batch(reads, target, k, q=Q):
    """predict() for every read against one target (converted and indexed once)"""
    tb = _bytes(target)
    index, present = build_index(tb, q), set(tb)
    return [predict(r, tb, k, index, present, q) for r in reads]


def seed_filter(qr, t, k, q=Q, index=None, caps=True):
    """(best, end columns) when the least windowed score is <= k, None when it is not (or the read has no window),
    "back" when a cap hands the read back"""
    qr = np.asarray(qr); t = np.asarray(t)
    diags = lookup(qr, t, k, q, index, caps)
    if diags == "back":
        return "back"
    ws = windows(diags, len(qr), k, len(t))
    if caps and any(b - a + 1 > MAX_WINDOW for a, b in ws):
        return "back"
    best, ends = None, []
    for a, b in ws:
        sc = bottom_row(qr, t[a:b + 1])                 # restarted at column a: D'[m][j] >= D[m][j]
        lo = int(sc.min())
        if lo > k or (best is not None and lo > best):
            continue
        cols = (np.nonzero(sc == lo)[0] + a).tolist()
        if best is None or lo < best:
            best, ends = lo, cols
        else:
            ends += cols
    return None if best is None else (best, ends)


def reference(qr, t, k):
    """the textbook DP: (best, every end column) when best <= k, else None"""
    sc = bottom_row(qr, t)
    b = int(sc.min())
    return (b, np.nonzero(sc == b)[0].tolist()) if b <= k else None
