"""Batches of tests/test_gpu_delay_rows8.py, built the same way by the test and by its child process
(tests/delay_rows8_child.py): the plain full-height kernel on rows built with SEVEN delay rows (scan_reads_kernel<NWD, 2, true, 7>,
DESIGN.md 3) at 1, 2, 5 and 8 words, and beside each a batch whose longest read leaves six free rows, which must keep the
three-row form.  HW, distance, k = -1, against T = 70,001 symbols (not a multiple of 16: the last segment ends in the ragged
tail, which follows the score at bit 24).

The kernel only sees the reads that the first level (threshold 8, banded kernel) leaves open, so every read here is more than
8 edits away from every window of the target, the planted ones included.  The target is uniform over A, C, G, T; a planted
read is J >= 10 symbols N, which nothing in the target matches, followed by an exact copy of the L = m - J symbols of the
target that end at a chosen column e.  Its distance is J, its end location is e, and over the last L columns of the window the
bottom-row score comes down by 1 per column into the hit: the steepest descent a group of eight columns can hold.  (A whole
exact copy resolves at the first level and never reaches this kernel; tests/test_delay_rows8_model.py runs it through the
model.)  Planted per batch (`planted`, by kind):
  "head"    windows ending at the columns 0 .. 7: N^(m - c - 1) and the first c + 1 symbols of the target (a tie with every
            other place where those symbols stand: thousands of end locations at c = 0);
  "tail"    windows ending at T - 1 .. T - 8;
  "group"   windows ending at every residue mod 8, junk copies and windows with ten substitutions to N;
  "seam"    windows ending at the last column of a segment, the first and the second of the next, and one that straddles the
            boundary, at the boundaries 1, 2 and 9 of the main launch (segments of SEG = 4,128 columns: the test asserts it);
  "pair"    the copy's last symbol substituted: columns e - 1 and e tie, both inside one group of eight;
  "twenty"  a window that stands 20 times inside ONE segment: the segment's own cap of 16 positions overflows;
  "live"    a window that stands exactly in segment 11 and with three substitutions (to other symbols of the target) in
            segment 2, and one the other way round: the better score comes from another segment (ReadScanArgs::liveBest).
Random reads are uniform over A, C, G, T (one word: N with probability 0.55, or no 25-mer would stay open); their lengths cycle
over the pads 7 .. 31 of the word count (one word: 18 .. 25, and one read each of 1 .. 17, which the first level resolves).

The last level takes the plain kernel only with at least 4,096 open slots: `batch` counts them with the reference on the CPU."""
import functools

import numpy as np

from pair_shift_cases import open_reads
from plain_column_cases import T

WORDS = (1, 2, 5, 8)
SEG = 4128                      # columns per segment of the main launch at T = 70,001 and 4,096 .. 8,191 lanes
NAMES = ["%d%s" % (n, s) for n in WORDS for s in ("", "s")]
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_N = np.uint8(ord("N"))
N_RANDOM = {1: 5600, 2: 4160, 5: 4160, 8: 4160}


def free_rows(name):
    """rows the longest read of the batch leaves free in its last word: 7 (the deep form) or 6 (the three-row form)"""
    return 6 if name.endswith("s") else 7


def words(name):
    return int(name.rstrip("s"))


def expected_depth(name):
    return 7 if free_rows(name) >= 7 else 3


def _target(rng):
    return _ACGT[rng.integers(0, 4, T)]


def _junk(m):
    return max(10, m // 3)


def _junk_copy(target, e, m):
    """J symbols N and the m - J symbols of the target that end at column e"""
    J = _junk(m)
    s = e - (m - J) + 1
    assert 0 <= s and e < T, (e, m)
    return np.ascontiguousarray(np.concatenate([np.full(J, _N), target[s:e + 1]]))


@functools.lru_cache(maxsize=None)
def batch(name):
    assert name in NAMES
    nwd, free = words(name), free_rows(name)
    rng = np.random.default_rng(4700 + 10 * nwd + free)
    hi = 32 * nwd - free
    lo = 32 * nwd - 31
    ls = list(range(18, hi + 1)) if nwd == 1 else list(range(lo, hi + 1))
    pl = ls[-3:] if nwd == 1 else [hi, ls[len(ls) // 2], hi - 1, ls[3]]          # lengths of the planted reads, in turn
    target = _target(rng)

    # windows written INTO the target first: the twenty copies and the two pairs of the liveBest reads
    mt = hi
    Lt = mt - _junk(mt)
    wt = _ACGT[rng.integers(0, 4, Lt)]
    twenty_ends = []
    at = 3 * SEG + 32
    for i in range(20):
        target[at:at + Lt] = wt
        twenty_ends.append(at + Lt - 1)
        at += Lt + 8 + i % 8
    assert at < 4 * SEG - 32 and len({e % 8 for e in twenty_ends}) >= 4
    live = []
    for far, near in ((11, 2), (5, 14)):                       # (segment of the exact copy, segment of the worse one)
        m = pl[1]
        L = m - _junk(m)
        w = _ACGT[rng.integers(0, 4, L)]
        worse = w.copy()
        for q in (L // 4, L // 2, 3 * L // 4):                # three substitutions (the target keeps to its four symbols)
            worse[q] = _ACGT[(int(np.searchsorted(_ACGT, worse[q])) + 1) % 4]
        target[far * SEG + 500:far * SEG + 500 + L] = w
        target[near * SEG + 700:near * SEG + 700 + L] = worse
        live.append((np.ascontiguousarray(np.concatenate([np.full(_junk(m), _N), w])), far * SEG + 500 + L - 1))

    planted = []                                               # (kind, read, a column that must be among its end locations)
    it = 0

    def length():
        nonlocal it
        it += 1
        return pl[it % len(pl)]

    for c in range(8):
        m = hi
        planted.append(("head", np.ascontiguousarray(np.concatenate([np.full(m - c - 1, _N), target[0:c + 1]])), c))
    for d in range(8):
        planted.append(("tail", _junk_copy(target, T - 1 - d, length()), T - 1 - d))
    for i in range(16):
        m = length()
        e = int(rng.integers(4 * SEG + 300, 16 * SEG)) // 8 * 8 + i % 8
        planted.append(("group", _junk_copy(target, e, m), e))
    for i in range(8):
        m = length()
        e = int(rng.integers(4 * SEG + 300, 16 * SEG)) // 8 * 8 + i % 8
        w = target[e - m + 1:e + 1].copy()
        w[rng.choice(m - 2, 10, replace=False)] = _N            # (the last two symbols stay: the window still ends at e)
        planted.append(("group", np.ascontiguousarray(w), e))
    for b in (1, 2, 9):
        for e in (b * SEG - 1, b * SEG, b * SEG + 1, b * SEG + 4):
            planted.append(("seam", _junk_copy(target, e, length()), e))
    for i in range(4):
        m = length()
        e = int(rng.integers(4 * SEG + 300, 16 * SEG)) // 8 * 8 + 1 + 2 * i
        r = _junk_copy(target, e, m)
        r[-1] = _ACGT[(int(np.searchsorted(_ACGT, r[-1])) + 1) % 4]
        planted.append(("pair", r, e))
    planted.append(("twenty", np.ascontiguousarray(np.concatenate([np.full(_junk(mt), _N), wt])), twenty_ends[0]))
    for r, e in live:
        planted.append(("live", r, e))

    def rand_read(m):
        if nwd == 1:
            r = _ACGT[rng.integers(0, 4, m)]
            r[rng.random(m) < 0.55] = _N
            return r
        return _ACGT[rng.integers(0, 4, m)]

    reads = [rand_read(ls[i % len(ls)]) for i in range(N_RANDOM[nwd])]
    if nwd == 1:
        reads += [rand_read(m) for m in range(1, 18)]
    step = len(reads) // len(planted)
    for i, (_, r, _e) in enumerate(planted):                   # spread through the batch rather than in a block of their own
        assert 1 <= len(r) <= hi, len(r)
        reads.insert((step + 1) * i + 7, r)
    assert len(reads) < 8192                                    # (SEG holds for 4,096 .. 8,191 lanes; the first threshold below 16,384 slots)
    assert max(len(r) for r in reads) == hi and set(range(lo, hi + 1)) <= {len(r) for r in reads}
    n_open = open_reads(reads, target)
    assert 4096 <= n_open, (name, n_open)
    return {"reads": reads, "target": target, "open": n_open, "planted": planted, "twenty_ends": twenty_ends}
