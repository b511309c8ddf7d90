"""Planted inputs for the exact k-mer seed filter (edlib_amd/csrc/reads_seed.hip), shared by the CPU tests
(tests/test_seed_model.py: every case does what it claims, on a target of a few thousand columns, against the textbook DP)
and the GPU tests (tests/test_gpu_seed_filter.py: the same structures on targets of 131,072 .. 256,001 columns).  numpy only,
every generator seeded.

A Planter owns (or shares) a random four-symbol target and writes planted structures into regions of its own, at least
RESERVE columns away from both target ends and a read's window apart from each other.  Every planted read comes with a claim:
a dict of what seed_model.predict() must say about it ("diagonals", "columns", "back", "bucket", "window") and, under
"found", whether the textbook DP finds it within k ("dist": at exactly that distance).  Claims are exact on the small targets
of the CPU tests; on a target of 256,000 columns a random extra hit is possible, so the GPU tests take their expectations
from the model and only re-check the claims of the cap cases.

The window-cap cases reach 1024 and 1025 columns exactly for every (word count, k) the tests use (the gaps between the
copies are free between a piece's length and m + 2k: asserted in window_cap), but for one: reads of 32 bases at k = 0 reach
1024 columns with exactly 32 diagonals and cannot go beyond (a 33rd diagonal trips the other cap), so that pair has no
window of 1025."""
import numpy as np

from seed_model import BUCKET_CAP, MAX_DIAG, MAX_WINDOW, Q, pieces

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# the shortest read of every word count in the GPU batches: k_f = 1 / 3 / 5 / 7 / 8 / 11 / 13 / 16 at T = 256,000
M_MIN = {1: 24, 2: 48, 3: 72, 4: 108, 5: 129, 6: 161, 7: 193, 8: 225}
RESERVE = 640               # columns at both target ends that no region touches (two windows of the longest read)

GENERATORS = ("word_edges", "target_ends", "compare_tails", "diag_32", "diag_33", "bucket_64", "bucket_65", "window_1024",
              "window_1025", "absent_bytes")


def _mutate(rng, w, edits, at):
    """`edits` edits of w at the query positions `at` (cycled), kinds cycling substitution / insertion / deletion"""
    w = w.copy()
    for e in range(edits):
        p = int(min(max(at[e % len(at)], 0), len(w) - 1))
        kind = (e + int(rng.integers(0, 3))) % 3
        if kind == 0:
            w[p] = _ACGT[(np.searchsorted(_ACGT, w[p]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            w = np.insert(w, p, _ACGT[rng.integers(0, 4)])
        else:
            w = np.delete(w, p)
    return np.ascontiguousarray(w)


def _reads(target, n, seed, kf, mlo=131, mhi=158, unrelated=0.05, above=0.03, with_n=0.02, avoid=None):
    """n reads of mlo..mhi bases: copies of the target with 0..kf edits, many on the boundaries of the kf + 1 pieces, on
    the first and the last base and as indels at both ends; `above` of them with kf + 1 or kf + 2 edits, `unrelated` of
    them random, `with_n` of them holding an N; reads at the target's first and last columns.  avoid = (lo, hi): no read
    is copied from these columns (a Planter's regions: their repeats are for the planted reads alone)"""
    rng = np.random.default_rng(seed)
    T = len(target)
    out = []
    for i in range(n):
        m = int(rng.integers(mlo, mhi + 1))
        u = rng.random()
        if u < unrelated:
            out.append(np.ascontiguousarray(_ACGT[rng.integers(0, 4, m)]))
            continue
        s = 0 if i % 97 == 0 else (T - m if i % 97 == 1 else int(rng.integers(0, T - m)))
        while avoid is not None and s + m > avoid[0] and s < avoid[1]:
            s = int(rng.integers(0, T - m))
        w = target[s:s + m]
        edits = int(rng.integers(kf + 1, kf + 3)) if u < unrelated + above else int(rng.integers(0, kf + 1))
        L = m // (kf + 1)
        bounds = [j * L for j in range(1, kf + 1)] + [j * L - 1 for j in range(1, kf + 1)]
        style = i % 4
        if style == 0 and bounds:
            at = bounds
        elif style == 1:
            at = [0, m - 1] + bounds
        elif style == 2 or not bounds:
            at = [0, m - 1]
        else:
            at = list(rng.integers(0, m, max(1, edits)))
        rng.shuffle(at)
        w = _mutate(rng, w, edits, at)
        if rng.random() < with_n:
            w = w.copy()
            w[int(rng.integers(0, len(w)))] = ord("N")
        out.append(w)
    return out


def fit_lengths(reads, mlo, mhi, seed):
    """indels may have moved a read out of its word count: cut it, or extend it with random bases"""
    rng = np.random.default_rng(seed)
    out = []
    for r in reads:
        if len(r) > mhi:
            r = r[:mhi]
        elif len(r) < mlo:
            r = np.concatenate([r, _ACGT[rng.integers(0, 4, mlo - len(r))]])
        out.append(np.ascontiguousarray(r))
    return out


class Planter:
    def __init__(self, nwd, T, k, seed, mlo=None, target=None, start=None, many_locations=True):
        """reads of `nwd` words (mlo .. 32 nwd bases, mlo default the least the word count and 12 (k + 1) allow) for a seed
        pass at threshold k.  `target`: a shared target to plant into (regions from `start` on) instead of a fresh random
        one.  many_locations=False keeps every read at 16 end locations or fewer (k = 0 makes every copy a full one)."""
        self.nwd, self.T, self.k = nwd, int(T), k
        self.mhi = 32 * nwd
        self.mlo = max(32 * (nwd - 1) + 1, Q * (k + 1)) if mlo is None else mlo
        assert Q * (k + 1) <= self.mlo <= self.mhi and self.mlo > 32 * (nwd - 1)
        self.rng = np.random.default_rng(seed)
        self.target = _ACGT[self.rng.integers(0, 4, self.T)].copy() if target is None else target
        assert len(self.target) == self.T
        self.span = self.mhi + 2 * k + 2                   # a read's window and a column on either side
        self.cur = RESERVE if start is None else start
        self.many_locations = many_locations
        self.reads, self.claims = [], []

    # ---------------------------------------------------------------------------------------------------- tools
    def _region(self, n):
        s = self.cur + self.span
        self.cur = s + n
        assert self.cur + self.span + RESERVE <= self.T, "the target is too short for the planted cases"
        return s

    def _fresh(self, n):
        return _ACGT[self.rng.integers(0, 4, n)]

    def _other(self, c):
        return _ACGT[(int(np.searchsorted(_ACGT, c)) + 1 + int(self.rng.integers(0, 3))) % 4]

    def _add(self, read, **claim):
        assert self.mlo <= len(read) <= self.mhi, (len(read), self.mlo, self.mhi)
        self.reads.append(np.ascontiguousarray(read, dtype=np.uint8))
        self.claims.append(claim)

    def edge_lengths(self):
        """m = 32 NWD, 32 NWD - 1 and the shortest length of the word count: bit (m - 1) & 31 = 31, 30 and (from five
        words on, where 32 (NWD - 1) + 1 bases hold the pieces) 0"""
        return sorted({self.mhi, max(self.mlo, self.mhi - 1), self.mlo})

    def _split_length(self):
        """the longest length whose pieces come in both sizes, L and L + 1"""
        for m in range(self.mhi, self.mlo - 1, -1):
            if m % (self.k + 1):
                return m
        return self.mhi

    def _tail_lengths(self):
        """the lengths compare_tails plants: one whose pieces come in both sizes, and one for every len - 12 of 0, 1, 15, 16,
        17, 31, 32 (nothing, one symbol, a chunk but one, a whole chunk, a chunk and one, ...) that this word count and k reach"""
        want, out = {0, 1, 15, 16, 17, 31, 32}, [self._split_length()]
        for m in range(self.mlo, self.mhi + 1):
            got = {n - Q for _, n in pieces(m, self.k)} & want
            if got:
                want -= got
                out.append(m)
        return sorted(set(out))

    # ------------------------------------------------------------------------------------------------ generators
    def word_edges(self):
        """clean copies at the three edge lengths (k + 1 hits on ONE diagonal), and edits on the last row: a substitution
        of the last base, the target's column under the last base deleted"""
        k = self.k
        for m in self.edge_lengths():
            w = self._fresh(m + 1)
            s = self._region(m + 1)
            self.target[s:s + m + 1] = w
            self._add(w[:m], diagonals=1, columns=m + 2 * k, back=False, found=True, dist=0)
            r = w[:m].copy()
            r[m - 1] = self._other(r[m - 1])
            if k >= 1:
                self._add(r, diagonals=1, columns=m + 2 * k, back=False, found=True, dist=1)
                self._add(np.delete(w, m - 1), diagonals=1, columns=m + 2 * k, back=False, found=True)
            else:
                self._add(r, diagonals=0, columns=0, back=False, found=False)

    def target_ends(self):
        """hits at P = 0 and with P + len = T, alone and with every other piece edited; reads hanging over column 0 and
        column T - 1 by 1 .. k bases; a key in the last len - 1 positions (P + len > T: no hit)"""
        k, T, t = self.k, self.T, self.target
        for m in sorted({self.mhi, self.mlo}):
            ps = pieces(m, k)
            self._add(t[:m].copy(), diagonals=1, columns=m + k, back=False, found=True, dist=0)
            self._add(t[T - m:].copy(), diagonals=1, columns=m + k, back=False, found=True, dist=0)
            if k >= 1:
                r = t[:m].copy()                               # only the first piece is intact: its one hit has P = 0
                for o, n in ps[1:]:
                    r[o + n // 2] = self._other(r[o + n // 2])
                self._add(r, diagonals=1, columns=m + k, back=False, found=True)
                r = t[T - m:].copy()                           # only the last piece: P + len = T exactly
                for o, n in ps[:-1]:
                    r[o + n // 2] = self._other(r[o + n // 2])
                self._add(r, diagonals=1, columns=m + k, back=False, found=True)
            for h in sorted({h for h in (1, (k + 1) // 2, k) if 1 <= h <= k}):
                self._add(np.concatenate([self._fresh(h), t[:m - h]]), diagonals=1, columns=m - h + k, back=False, found=True)
                self._add(np.concatenate([t[T - m + h:], self._fresh(h)]), diagonals=1, columns=m - h + k, back=False, found=True)
            o, n = ps[-1]
            for j in sorted({Q, n - 1}):
                if j < Q or j >= n:
                    continue
                r = self._fresh(m)                             # the last piece begins like the target's last j columns
                r[o:o + j] = t[T - j:]
                r[o + j:] = t[:T].min()                        # ... and goes on with the symbol a zeroed stream would hold
                self._add(r, diagonals=0, columns=0, back=False, found=False)

    def compare_tails(self):
        """a first, a middle and the last piece of a read (lengths L + 1 and L), each planted once exactly and followed by a
        mismatch at offset len (a diagonal), and as near misses with ONE symbol changed at offset 12, at every later start
        of a 16-symbol chunk and at offset len - 1 (in the bucket, never a diagonal)"""
        k = self.k
        for m, i in [(m, i) for m in self._tail_lengths() for i in sorted({0, k // 2, k})]:
            o, n = pieces(m, k)[i]
            r = self._fresh(m)
            piece = r[o:o + n].copy()
            s = self._region(n + 1)
            self.target[s:s + n] = piece
            self.target[s + n] = self._other(r[o + n]) if o + n < m else self._fresh(1)[0]
            offs = sorted({x for x in [Q, n - 1] + list(range(Q + 16, n, 16)) if Q <= x < n})
            for off in offs:
                c = piece.copy()
                c[off] = self._other(c[off])
                s2 = self._region(n)
                self.target[s2:s2 + n] = c
            self._add(r, diagonals=1, columns=m + 2 * k, back=False, bucket=1 + len(offs))

    def many_diagonals(self, c):
        """c copies of a read of 32 NWD bases, m + 2k + 2 columns apart: c diagonals whose windows do not merge.  The first
        four are whole copies, the others hold one piece only (the read keeps few end locations); k = 0: every copy is whole"""
        k, m = self.k, self.mhi
        if k == 0 and not self.many_locations:
            c = min(c, 16)
        r = self._fresh(m)
        ps = pieces(m, k)
        stride = m + 2 * k + 2
        base = self._region(c * stride)
        for j in range(c):
            d = base + j * stride
            if j < 4 or k == 0:
                self.target[d:d + m] = r
            else:
                o, n = ps[j % (k + 1)]
                self.target[d + o:d + o + n] = r[o:o + n]
        over = c > MAX_DIAG
        self._add(r, diagonals=0 if over else c, columns=0 if over else c * (m + 2 * k), back=over, found=True, dist=0)

    def diag_32(self):
        self.many_diagonals(MAX_DIAG)

    def diag_33(self):
        self.many_diagonals(MAX_DIAG + 1)

    def bucket(self, count):
        """a read planted once, and count - 1 more occurrences of just the first 12 symbols of its middle piece (the 13th
        differs): a bucket of `count` positions, one diagonal"""
        k, m = self.k, self.mhi
        r = self._fresh(m)
        o, n = pieces(m, k)[k // 2]
        assert n > Q
        s = self._region(m)
        self.target[s:s + m] = r
        s2 = self._region(16 * (count - 1))
        for j in range(count - 1):
            a = s2 + 16 * j
            self.target[a:a + Q] = r[o:o + Q]
            self.target[a + Q] = self._other(r[o + Q])
        over = count > BUCKET_CAP
        self._add(r, bucket=count, diagonals=0 if over else 1, columns=0 if over else m + 2 * k, back=over, found=True, dist=0)

    def bucket_64(self):
        self.bucket(BUCKET_CAP)

    def bucket_65(self):
        self.bucket(BUCKET_CAP + 1)

    def window_cap(self, total):
        """copies of the middle piece of a read of 32 NWD bases (k = 0: of the read) on at least four diagonals so close that
        their windows merge into ONE window of exactly `total` columns -- or, where no spacing gives that (k = 0: whole reads
        back to back, the window is a multiple of m), of the closest length on the same side of the cap: 1152 / 1280 columns
        instead of 1025 for reads of 128 / 256 bases at k = 0.  The claim says which."""
        k, m = self.k, self.mhi
        o, n = pieces(m, k)[k // 2]
        gmin, gmax = n, m + 2 * k                              # copies back to back .. windows that just touch
        for total in (range(total, total + 2 * m) if total > MAX_WINDOW else range(total, m, -1)):
            D = total - m - 2 * k                              # from the first diagonal to the last
            ngap = max(3, -(-D // gmax))
            if gmin <= D // ngap and -(-D // ngap) <= gmax:
                break
        else:
            raise AssertionError((m, k, total))
        if k == 0 and ngap + 1 > 16 and not self.many_locations:
            return                                             # (every copy is an end location at distance 0)
        if ngap + 1 > MAX_DIAG:
            return                                             # (32 bases, k = 0: 32 diagonals span 1024 columns at most)
        r = self._fresh(m)
        base = self._region(D + m)
        d = base
        for j in range(ngap + 1):
            self.target[d + o:d + o + n] = r[o:o + n]
            d += D // ngap + (1 if j < D % ngap else 0)
        over = total > MAX_WINDOW
        self._add(r, window=total, diagonals=0 if over else ngap + 1, columns=0 if over else total, back=over)

    def window_1024(self):
        self.window_cap(MAX_WINDOW)

    def window_1025(self):
        self.window_cap(MAX_WINDOW + 1)

    def absent_bytes(self):
        """a byte the target lacks inside the first, a middle and the last piece of a planted read"""
        k = self.k
        for m, i in zip((self.mlo, self._split_length(), self.mhi), (0, k // 2, k)):
            w = self._fresh(m)
            s = self._region(m)
            self.target[s:s + m] = w
            o, n = pieces(m, k)[i]
            r = w.copy()
            r[o + n // 2] = ord("N")
            if k >= 1:
                self._add(r, diagonals=1, columns=m + 2 * k, back=False, found=True, dist=1)
            else:
                self._add(r, diagonals=0, columns=0, back=False, found=False)

    def plant(self, over_caps=True):
        """every generator; over_caps=False leaves out the three that are handed back"""
        for name in GENERATORS:
            if over_caps or name not in ("diag_33", "bucket_65", "window_1025"):
                getattr(self, name)()
        return self


def claims_hold(claims, pred, keys=("back", "diagonals", "columns", "bucket", "window")):
    """the claimed keys of predict()'s answer, read by read: [] or what differs"""
    bad = []
    for i, (c, p) in enumerate(zip(claims, pred)):
        for key in keys:
            if c is not None and key in c and c[key] != p[key]:
                bad.append((i, key, c[key], p[key]))
    return bad


# ------------------------------------------------------------------------------------------- the GPU tests' batches
# Each returns {"reads", "target", "k", "task", "claims" (None for the filler reads), "K": {word count: the seed pass's
# threshold}}; the child processes of the GPU tests and their parents build the same batch from the same name.

def _target_length(T, nwd):
    """T mod 16 = 0, 1 or 15 by word count: the packed stream's last dword, the last indexed position T - 12"""
    return T + (0, 1, -1)[nwd % 3]


def single_group(nwd, k, T=256_000, n=4_400, seed=0, mlo=None, over_caps=False, many_locations=False, task="distance",
                 caller_k=None):
    """one word count: every planted case and filler reads with 0 .. k + 2 edits up to n reads (n is no multiple of 64:
    the last wave is padded)"""
    T = _target_length(T, nwd)
    P = Planter(nwd, T, k, 7000 + 100 * nwd + k + seed, mlo=mlo, many_locations=many_locations).plant(over_caps)
    fill = fit_lengths(_reads(P.target, n - len(P.reads), 7001 + 100 * nwd + k + seed, k, P.mlo, P.mhi,
                              avoid=(RESERVE, P.cur + P.span)), P.mlo, P.mhi, seed)
    assert n % 64 and len(fill) > 0
    return {"reads": P.reads + fill, "target": P.target, "k": k if caller_k is None else caller_k, "task": task,
            "claims": P.claims + [None] * len(fill), "K": {nwd: k}}


def several_groups(words, ks, T, n_each, seed, caller_k, extra=(), over_caps=True):
    """one shared target, a planted group per word count (threshold ks[nwd]), units in random order; `extra`: more reads"""
    rng = np.random.default_rng(seed)
    target = _ACGT[rng.integers(0, 4, T)].copy()
    reads, claims, cur = [], [], RESERVE
    planters = []
    for nwd in words:
        P = Planter(nwd, T, ks[nwd], seed + nwd, mlo=max(M_MIN[nwd], Q * (ks[nwd] + 1)), target=target, start=cur).plant(over_caps)
        cur = P.cur
        planters.append(P)
    for P in planters:                                         # (the filler copies the target as planted)
        fill = fit_lengths(_reads(target, n_each - len(P.reads), seed + 50 + P.nwd, P.k, P.mlo, P.mhi,
                                  avoid=(RESERVE, cur + P.span)), P.mlo, P.mhi, seed)
        reads += P.reads + fill
        claims += P.claims + [None] * len(fill)
    reads += [np.ascontiguousarray(x) for x in extra]
    claims += [None] * len(extra)
    order = rng.permutation(len(reads))
    return {"reads": [reads[i] for i in order], "target": target, "k": caller_k, "task": "distance",
            "claims": [claims[i] for i in order], "K": dict(ks)}


def three_symbols(nwd=5, k=8, T=256_000, n=4_400, seed=9100):
    """a target of A, C and G; a third of the reads hold a T"""
    rng = np.random.default_rng(seed)
    target = _ACGT[rng.integers(0, 3, T)].copy()
    reads = fit_lengths(_reads(target, n, seed + 1, k, M_MIN[nwd], 32 * nwd), M_MIN[nwd], 32 * nwd, seed)
    for i in range(0, n, 3):
        reads[i][int(rng.integers(0, len(reads[i])))] = ord("T")
    return {"reads": reads, "target": target, "k": k, "task": "distance", "claims": [None] * n, "K": {nwd: k}}


def two_symbols(nwd=8, k=3, T=256_000, n=4_400, seed=9200):
    """a random target of A and C: buckets of about T / 4096 positions (62.5: both sides of the cap of 64)"""
    rng = np.random.default_rng(seed)
    target = _ACGT[rng.integers(0, 2, T)].copy()
    mlo = 32 * (nwd - 1) + 1
    reads = fit_lengths(_reads(target, n, seed + 1, k, mlo, 32 * nwd), mlo, 32 * nwd, seed)
    return {"reads": reads, "target": target, "k": k, "task": "distance", "claims": [None] * n, "K": {nwd: k}}


def low_complexity(nwd=5, k=8, T=256_000, n=4_400, seed=9300):
    """four symbols, a homopolymer run of 3,000 and a tandem repeat (unit of 5) of 4,000 columns (a tenth / an eighth of a
    shorter target); reads from inside both, across their four edges, and everywhere else"""
    rng = np.random.default_rng(seed)
    target = _ACGT[rng.integers(0, 4, T)].copy()
    h0, s0, hn, sn = T // 5, T // 2, min(3_000, T // 10), min(4_000, T // 8)
    target[h0:h0 + hn] = ord("A")
    target[s0:s0 + sn] = np.resize(np.frombuffer(b"ACGGT", dtype=np.uint8), sn)
    mlo, mhi = M_MIN[nwd], 32 * nwd
    special = []
    for i in range(min(200, n // 2)):
        m = int(rng.integers(mlo, mhi + 1))
        at = [h0 + hn // 3, s0 + sn // 4, h0 - m // 2, h0 + hn - m // 2, s0 - m // 2, s0 + sn - m // 2][i % 6] + int(rng.integers(0, 40))
        special.append(_mutate(rng, target[at:at + m], int(rng.integers(0, k + 1)), list(rng.integers(0, m, k + 1))))
    reads = fit_lengths(special + _reads(target, n - len(special), seed + 1, k, mlo, mhi), mlo, mhi, seed)
    return {"reads": reads, "target": target, "k": k, "task": "distance", "claims": [None] * n, "K": {nwd: k}}


def five_symbols(nwd=5, T=256_000, n=4_400, seed=9400):
    """ACGTN: the banded first pass (no seed pass)"""
    rng = np.random.default_rng(seed)
    target = _ACGT[rng.integers(0, 4, T)].copy()
    target[rng.integers(0, T, 300)] = ord("N")
    reads = fit_lengths(_reads(target, n, seed + 1, 8, M_MIN[nwd], 32 * nwd), M_MIN[nwd], 32 * nwd, seed)
    return {"reads": reads, "target": target, "k": -1, "task": "distance", "claims": [None] * n, "K": {}}


def spread_distances(nwd=6, T=131_072, n=16_448, seed=9500, dmax=40):
    """reads with 0 .. dmax edits, evenly: most are above any k_f, the probe stays open and prices a ladder"""
    rng = np.random.default_rng(seed)
    target = _ACGT[rng.integers(0, 4, T)].copy()
    mlo, mhi = M_MIN[nwd], 32 * nwd
    reads = []
    for i in range(n):
        m = int(rng.integers(mlo, mhi + 1))
        s = int(rng.integers(0, T - m))
        e = i % (dmax + 1)
        reads.append(_mutate(rng, target[s:s + m], e, list(rng.integers(0, m, max(e, 1)))))
    return {"reads": fit_lengths(reads, mlo, mhi, seed), "target": target, "k": -1, "task": "distance", "claims": [None] * n,
            "K": {}}


def batch(name):
    """the batch of a child-process test by name"""
    from seed_model import seed_threshold
    kind, _, arg = name.partition(":")
    if kind == "caps":                                         # caps:<nwd>: the caller's k is k_f, caps crossed and not
        nwd = int(arg)
        T = _target_length(256_000, nwd)
        return single_group(nwd, seed_threshold(M_MIN[nwd], T), mlo=M_MIN[nwd], over_caps=True, many_locations=True, seed=3)
    if kind == "kminus1":                                      # groups of 4 .. 8 words against 200,000 columns, k = -1
        T = 200_000
        ks = {w: seed_threshold(M_MIN[w], T) for w in (4, 5, 6, 7, 8)}
        return several_groups((4, 5, 6, 7, 8), ks, T, 5_400, 8100, -1)
    if kind == "ineligible108":                                # 108 bases against 256,000 columns: k_f = 7 < 8
        b = single_group(4, 7, T=256_000, mlo=108, seed=5)
        b["k"], b["K"] = -1, {}
        return b
    return {"three": three_symbols, "two": two_symbols, "lowcomplexity": low_complexity, "five": five_symbols,
            "spread": spread_distances}[kind]()
