"""Batches of tests/test_gpu_wide_rows.py, built the same way by the test, by the CPU test of the cases
(tests/test_wide_rows_cases.py) and by the child process (tests/wide_rows_child.py): HW reads against shared targets of
exactly 8 and exactly 16 distinct bytes, which keep 8 / 16 Peq rows per word in LDS and run on scan_reads_banded_kernel
<N, 8|16> and scan_reads_full_kernel<N, 8|16>, and the 10- / 12- / 14- / 16-word groups of the full-height
kernel.

Targets: T = 70,001 columns (not a multiple of 16: the masked last block of a scan; at least 65,536: the last level's
4,096-column pre-scan runs), uniform ACGT, then
  rows8   ACGT + runs of N + scattered R, Y, K                                      (8 symbols)
  rows16  ACGTN + scattered R, Y, K, M, S, W, then soft-masked stretches: acgtn     (16 symbols)
Lower case is applied through ONE boolean mask, once per position, and only to ACGTN (overlapping stretches that each add 32
give a 17th symbol, and 17 symbols leave the reads-per-lane kernels altogether).  The masking reaches column T - 1.  Then
windows of the finished target are copied to other places of it (bytes copied, nothing added): one window stands 20 times
(3,200 columns apart: more end locations than the 16 positions a slot keeps, so the exact pass follows), one stands
twice at starts of different residues mod 4.  Those windows hold an N run and, on rows16, the edge of a lower-case stretch.

Full-height batches (`full`): uniform random ACGT reads, lengths over every pad of the word count, and 64 planted reads
spread through the batch: edited copies of target windows -- the window at column 0, the windows ending at T - 1 .. T - 4,
the 20-copy window, the twice-standing one, and windows anywhere.  The last level takes the full-height kernel only with at
least 4,096 open slots, and the batch must stay below 16,384 slots (from there a probe picks thresholds): the builder counts
with pair_shift_cases.open_reads and asserts both."""
import functools

import numpy as np

from plain_column_cases import T, _ACGT, _random
from pair_shift_cases import K_FIRST, open_reads
from pair_shift_cases import _edit as _edit_within

LAYOUTS = ("rows8", "rows16")
SYMS = {"base": 4, "rows8": 8, "rows16": 16}
ALPHABET = {"base": b"ACGT", "rows8": b"ACGTNRYK", "rows16": b"ACGTNRYKMSWacgtn"}
N_PLANTED = 64
N_COPIES = 20
COPY_AT = [3_000 + 3_200 * i for i in range(N_COPIES)]      # the 20-copy window; its source is the first
TWICE_AT = (1_501, 66_003)                                  # residues 1 and 3 mod 4
WORDS_FULL = tuple(range(1, 9))
WORDS_LONG = (10, 12)
# (word count, layout) of the fixed-k "locations" runs: a word count other than 2 and 5, and one whose whole height lies
# within the band of threshold 40 -- against unrelated sequence the score 96 rows down is about 40, so from four words on the
# band of k = 40 falls below the 85 % of the words at which the last level leaves the banded kernel.  (Run on an MI355X: seven
# and four words on rows16 both gave a level of 4,160 slots with plain=0; the last word's share of the columns, restated on the
# CPU for the level's 64-read sample: three words 1.00 on rows8 and 0.91 on rows16, four words 0.87 and 0.72.)
LOCATIONS_RUNS = ((3, "rows8"), (3, "rows16"))
K_LOCATIONS = 40


def _runs(rng, n, count, lo, hi):
    m = np.zeros(n, dtype=bool)
    for _ in range(count):
        s = int(rng.integers(0, n)); m[s:s + int(rng.integers(lo, hi + 1))] = True
    return m


def target(seed, layout, wlen):
    """the target of one case; `wlen`: length of the windows copied within it (the 20-copy and the twice-standing one)"""
    rng = np.random.default_rng(seed)
    t = _random(rng, T).copy()
    if layout != "base":
        nrun = _runs(rng, T, 70, 2, 30)
        nrun[T - 2:T] = True                                # the masking reaches column T - 1
        nrun[6:8] = True                                    # and stands in the window at column 0
        nrun[COPY_AT[0] + 5:COPY_AT[0] + 8] = True          # an N run inside the 20-copy window and the twice-standing one
        nrun[TWICE_AT[0] + 3:TWICE_AT[0] + 5] = True
        t[nrun] = ord("N")
        codes = np.frombuffer(ALPHABET[layout][5:11], dtype=np.uint8)          # RYK / RYKMSW
        at = np.nonzero(rng.random(T) < 0.006 * len(codes))[0]
        at = at[at < T - 4]
        t[at] = codes[rng.integers(0, len(codes), len(at))]
    if layout == "rows16":
        lower = _runs(rng, T, 60, 40, 900)
        lower[T - 40:T] = True
        lower[COPY_AT[0]:COPY_AT[0] + 12] = True            # both windows start inside a stretch and leave it
        lower[TWICE_AT[0]:TWICE_AT[0] + 9] = True
        lower[12:40] = True                                 # and so does the window at column 0
        lower &= np.isin(t, np.frombuffer(b"ACGTN", dtype=np.uint8))
        t[lower] += 32                                      # once per position
    for s in COPY_AT[1:]:
        t[s:s + wlen] = t[COPY_AT[0]:COPY_AT[0] + wlen]
    t[TWICE_AT[1]:TWICE_AT[1] + wlen] = t[TWICE_AT[0]:TWICE_AT[0] + wlen]
    assert len(set(t.tolist())) == SYMS[layout], (layout, len(set(t.tolist())))
    return np.ascontiguousarray(t)


def lengths_full(nwd):
    return list(range(32 * nwd - 31, 32 * nwd + 1)) if nwd <= 8 else list(range(32 * nwd - 63, 32 * nwd + 1))


def _random_lengths(nwd):
    """lengths of the random reads, in batch order.  Every pad of the word count occurs; where short reads resolve at the
    first level (threshold 8) whatever they hold, most reads take the long lengths of the four-symbol recipes
    (plain_column_cases.batch_b: 31 and 32 of 7,488 for one word; pair_shift_cases: 48..64 for two)"""
    ls = lengths_full(nwd)
    if nwd == 1:
        return [ls[(i // 3) % 32] if i % 3 == 0 else 31 + i % 2 for i in range(7488)]
    if nwd == 2:
        return [33 + (i // 8) % 15 if i % 8 == 0 else 48 + i % 17 for i in range(4800)]
    return [ls[i % len(ls)] for i in range(4096)]


def _substitute(rng, w, nsub):
    """nsub substitutions at distinct positions that hold a base in either case (N and the IUPAC codes of the window stay)"""
    w = w.copy()
    at = np.nonzero(np.isin(w, np.frombuffer(b"ACGTacgt", dtype=np.uint8)))[0]
    for p in rng.choice(at, nsub, replace=False):
        w[p] = _ACGT[(int(np.searchsorted(_ACGT, w[p])) + 1 + int(rng.integers(0, 3))) % 4]
    return w


def _planted(rng, t, nwd):
    """64 edited copies of windows of t: 12..40 substitutions, insertions and deletions as in pair_shift_cases, but no more
    than two fifths of the window (a 64-row read with 40 edits is no copy of anything).  One word: 9..11 substitutions, which
    unlike as many mixed edits leave a 32-row read above the first level's threshold of 8, so that it is the full-height
    level that scans it.  The 20-copy read takes 12 substitutions (10 in one word) for the same reason.  Every other window
    anywhere is laid around an occurrence of one of the target's symbols beyond ACGT, each in turn."""
    ls = lengths_full(nwd)
    lo, hi = ls[0], ls[-1]
    wlen = window_length(nwd)

    def edit(w, i, keep=0):
        """(keep: symbols at either end of the window that stay, so that the alignment begins and ends where the window does)"""
        if keep > 0:
            return np.concatenate([w[:keep], edit(w[keep:-keep], i, -keep), w[-keep:]])
        if nwd == 1:
            return _substitute(rng, w, 9 if keep else 9 + i % 3)
        return _edit_within(rng, w, min(12 + i % 29, 2 * len(w) // 5), lo + 2 * keep, hi + 2 * keep)
    out = [edit(t[0:wlen], 2, 4)]
    for j in range(4):
        out.append(edit(t[T - j - wlen:T - j], 1 + j, 4))
    out.append(_substitute(rng, t[COPY_AT[0]:COPY_AT[0] + wlen], 10 if nwd == 1 else 12))
    out.append(edit(t[TWICE_AT[0]:TWICE_AT[0] + wlen], 1, 4))
    others = sorted(set(t.tolist()) - set(_ACGT.tolist()))
    bases = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    i = 0
    while len(out) < N_PLANTED:
        m = int(rng.integers(max(lo + 10, hi - 4), hi - 1)) if nwd <= 2 else int(rng.integers(lo + 10, hi - 1))
        s = int(rng.integers(0, T - m))
        if others and i % 2 == 0:
            at = np.nonzero(t[m:T - m] == others[(i // 2) % len(others)])[0] + m
            s = int(at[rng.integers(0, len(at))]) - int(rng.integers(0, m))
        if np.count_nonzero(np.isin(t[s:s + m], bases)) < 2 * m // 3:
            continue                                        # (mostly N: nothing to edit, and nothing that places the read)
        out.append(edit(t[s:s + m], i))
        i += 1
    for r in out:
        assert lo <= len(r) <= hi, len(r)
    return out


def window_length(nwd):
    ls = lengths_full(nwd)
    return ls[-1] - 2 if nwd <= 2 else (ls[0] + ls[-1]) // 2


def planted_at(n_random):
    """batch positions of the planted reads: spread through the batch rather than in a block of their own"""
    step = (n_random + N_PLANTED) // N_PLANTED
    return [step * i + 7 for i in range(N_PLANTED)]


@functools.lru_cache(maxsize=None)
def full(nwd, layout, count=True):
    """one group of nwd words that leaves at least 4,096 reads open above the first threshold (counted when `count`)"""
    assert nwd in WORDS_FULL + WORDS_LONG and layout in SYMS
    seed = 5100 + 20 * nwd + SYMS[layout]
    t = target(seed, layout, window_length(nwd))
    rng = np.random.default_rng(seed + 1)
    reads = [_random(rng, m) for m in _random_lengths(nwd)]
    at = planted_at(len(reads))
    for p, r in zip(at, _planted(rng, t, nwd)):
        reads.insert(p, r)
    assert {len(r) for r in reads} == set(lengths_full(nwd))
    b = {"reads": reads, "target": t, "planted": at, "nwords": nwd, "syms": SYMS[layout]}
    if count:
        b["open"] = open_reads(reads, t)
        assert b["open"] >= 4096 and (len(reads) + 63) // 64 * 64 < 16384, (nwd, layout, b["open"], len(reads))
    return b


@functools.lru_cache(maxsize=None)
def long_on_sixteen_rows():
    """reads of 257..384 bases against 16 symbols: no 10- / 12-word group there (64 KB of LDS rows per wave), the piece
    filter takes them"""
    t = target(5400, "rows16", window_length(12))
    rng = np.random.default_rng(5401)
    reads = [_random(rng, 257 + (5 * i) % 128) for i in range(192)]
    for p, r in zip(range(3, 192, 3), _planted(rng, t, 10) + _planted(rng, t, 12)):
        reads.insert(p, r)
    return {"reads": reads, "target": t}


def _related(t, lengths, seed, max_err, unrelated_every=0):
    from test_gpu_long_reads import _reads
    return _reads(t, lengths, seed, unrelated_every=unrelated_every, max_err=max_err)


@functools.lru_cache(maxsize=None)
def handed_back():
    """385..512 bases against 8 symbols: the piece filter hands the unrelated ones back to the 14- and 16-word groups of the
    full-height kernel (Batch::runLongReads)"""
    t = target(5500, "rows8", 400)
    rng = np.random.default_rng(5501)
    reads = [_random(rng, (385, 448, 449, 512)[i % 4]) for i in range(320)]
    for p, r in zip(range(2, 400, 5), _related(t, [385, 400, 448, 449, 480, 512] * 10, 5502, 0.1)):
        reads.insert(p, r)
    return {"reads": reads, "target": t}


@functools.lru_cache(maxsize=None)
def banded(nwd, layout):
    """400 windows of the target with indels and substitutions at per-read rates spread over 0..0.35 (every eleventh read is
    random), at every pad of the word count: fewer than 4,096 open, so the last level stays on the banded kernel and walks it
    through every band height"""
    assert nwd in WORDS_FULL and layout in LAYOUTS
    seed = 5600 + 20 * nwd + SYMS[layout]
    t = target(seed, layout, window_length(nwd))
    ls = lengths_full(nwd)
    reads = _related(t, [ls[i % 32] for i in range(400)], seed + 1, 0.35, unrelated_every=11)
    return {"reads": reads, "target": t, "nwords": nwd, "syms": SYMS[layout]}


def case(name):
    """a case by its name on the child's command line: kind:words:layout:task:k"""
    kind, nwd, layout, task, k = name.split(":")
    if kind == "full":
        b = full(int(nwd), layout, False)
    elif kind == "banded":
        b = banded(int(nwd), layout)
    else:
        b = {"long16": long_on_sixteen_rows, "back": handed_back}[kind]()
    return dict(b, task=task, k=int(k))


# ------------------------------------------------------------------------------------------ the reference's view of a batch

def reference(reads, t, task, k=-1):
    from oracle import oracle as O
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    return O.pool_align(np.concatenate(reads), qoff, t, np.array([0, len(t)], dtype=np.int64), True, "HW", task, k)


def matched_symbols(read, t, start, end, ops):
    """target bytes at the matching positions of one alignment (edlib's operations: 0 match, 1 a read symbol alone, 2 a
    target symbol alone, 3 mismatch); checks the walk against both sequences on the way"""
    qi, ti, out = 0, int(start), set()
    for op in ops.tolist():
        if op == 0:
            assert read[qi] == t[ti]
            out.add(int(t[ti]))
        elif op == 3:
            assert read[qi] != t[ti]
        qi += op != 2
        ti += op != 1
    assert qi == len(read) and ti == int(end) + 1, (qi, ti, len(read), end)
    return out
