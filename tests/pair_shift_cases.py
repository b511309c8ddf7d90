"""Batches of tests/test_gpu_pair_shift.py, built the same way by the test and by its child process
(tests/pair_shift_child.py): one per word count of the plain full-height kernel on bottom-aligned rows other than five
(five words at every pad is batch A of tests/plain_column_cases.py).  HW, distance, k = -1, against T = 70,001 symbols as
there.  Uniform random reads whose lengths cycle over every pad of the word count (32 nwd - 31 .. 32 nwd; two words: 48..64
only, shorter random reads mostly resolve at the first level), and 64 reads planted with 12..40 edits spread through the
batch, one window starting at column 0 and one ending at column T - 1.

The last level takes the plain kernel only with at least 4,096 open slots: `batch` counts, with the reference on the CPU, the
reads whose distance is above the first level's threshold (8 below 16,384 slots, engine_reads.hip) and asserts that there
are that many."""
import functools
import os
import sys

import numpy as np

from plain_column_cases import T, _ACGT, _random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORDS = (2, 3, 4, 6, 7, 8)
K_FIRST = 8
N_PLANTED = 64
# random reads per batch: by the reference a uniform random read of 48 symbols or more is practically never within 8 edits of
# a window of 70,001 random columns (two words: 3 of 4,672 reads were, planted ones included), so 4,096 random reads and the
# planted ones leave about 60 to spare over 4,096.  `batch` asserts the count.
N_RANDOM = {nwd: 4096 for nwd in WORDS}


def lengths(nwd):
    return list(range(48 if nwd == 2 else 32 * nwd - 31, 32 * nwd + 1))


def _edit(rng, w, nedit, lo, hi):
    """nedit substitutions, insertions and deletions, drawn one after the other; the length stays within lo..hi"""
    w = w.copy()
    for _ in range(nedit):
        p = int(rng.integers(0, len(w)))
        kind = int(rng.integers(0, 3))
        if kind == 1 and len(w) <= lo:
            kind = 2
        elif kind == 2 and len(w) >= hi:
            kind = 1
        if kind == 0:
            w[p] = _ACGT[(int(np.searchsorted(_ACGT, w[p])) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            w = np.delete(w, p)
        else:
            w = np.insert(w, p, _ACGT[rng.integers(0, 4)])
    return np.ascontiguousarray(w)


def open_reads(reads, target):
    """how many reads the reference leaves above the first level's threshold (HW distance > K_FIRST)"""
    from oracle import oracle as O
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    ref = O.pool_align(np.concatenate(reads), qoff, target, np.array([0, len(target)], dtype=np.int64), True, "HW",
                       "distance", K_FIRST)
    return int(np.count_nonzero(np.asarray(ref["editDistance"]) < 0))


@functools.lru_cache(maxsize=None)
def batch(nwd):
    assert nwd in WORDS
    rng = np.random.default_rng(4300 + nwd)
    target = _random(rng, T)
    ls = lengths(nwd)
    lo, hi = ls[0], ls[-1]
    reads = [_random(rng, ls[i % len(ls)]) for i in range(N_RANDOM[nwd])]
    mid = (lo + hi) // 2
    planted = [_edit(rng, target[0:mid], 14, lo, hi), _edit(rng, target[T - mid:T], 13, lo, hi)]
    for i in range(N_PLANTED - 2):
        m = int(rng.integers(lo + 2, hi - 1))
        s = int(rng.integers(0, T - m))
        planted.append(_edit(rng, target[s:s + m], 12 + i % 29, lo, hi))
    for i, r in enumerate(planted):                       # spread through the batch rather than in a block of their own
        assert lo <= len(r) <= hi, len(r)
        reads.insert(65 * i + 7, r)
    assert len(reads) == N_RANDOM[nwd] + N_PLANTED <= 4700
    assert {len(r) for r in reads} == set(ls)
    n_open = open_reads(reads, target)
    assert n_open >= 4096, (nwd, n_open)
    return {"reads": reads, "target": target, "open": n_open}
