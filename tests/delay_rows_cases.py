"""Batches of tests/test_gpu_delay_rows.py, built the same way by the test and by its child process
(tests/delay_rows_child.py): one per word count of the plain full-height kernel on rows built with delay rows
(scan_reads_kernel<NWD, 2, true, true>).  HW, distance, k = -1, against T = 70,001 symbols (not a multiple of 16:
the last segment ends in the ragged tail, which follows the score at bit 28).

Every read leaves the three delay rows their room: lengths cycle over the pads 3..31 of the word count (32 nwd - 31 ..
32 nwd - 3).  One and two words keep to the longer of those lengths, 26..29 and 48..61: shorter uniform random reads are
within the first level's threshold of some window of 70,001 random columns and never reach the last level (as in
tests/pair_shift_cases.py).  One word takes 12,000 reads, every other one of 29 symbols: by the reference 59 % of the random
29-mers, 24 % of the 28-mers, 4 % of the 27-mers and none of the 26-mers stay open.  64 planted reads with 12..40 edits are spread
through the batch:
  * one whose window starts at column 0, four whose windows end at T - 1, T - 2, T - 3 and T - 4;
  * four whose window stands twice in the target, the copies a different distance mod 4 apart: equal best scores in two
    different groups of four columns, at different places in their groups;
  * the rest anywhere, their windows ending at every residue mod 4 in turn.

The last level takes the plain kernel only with at least 4,096 open slots: `batch` counts, with the reference on the CPU, the
reads whose distance is above the first level's threshold and asserts that there are that many.

"mixed" is batch A of tests/plain_column_cases.py: five words at every pad 0..31, so the group is not eligible and keeps the
bottom-aligned kernel without delay rows."""
import functools

import numpy as np

from pair_shift_cases import N_PLANTED, _edit, open_reads
from plain_column_cases import T, _random
import plain_column_cases as PC

WORDS = (1, 2, 3, 4, 5, 6, 8)
DELAY_ROWS = 3
N_RANDOM = {nwd: 4100 for nwd in WORDS}
N_RANDOM[1] = 12000


def lengths(nwd):
    """the cycle of the random reads' lengths"""
    if nwd == 1:
        return [29, 28, 29, 27, 29, 28, 29, 26]
    lo = 48 if nwd == 2 else 32 * nwd - 31
    return list(range(lo, 32 * nwd - DELAY_ROWS + 1))


@functools.lru_cache(maxsize=None)
def batch(nwd):
    assert nwd in WORDS
    rng = np.random.default_rng(4400 + nwd)
    target = _random(rng, T)
    ls = lengths(nwd)
    lo, hi = min(ls), max(ls)
    mid = (lo + hi) // 2
    # windows that stand twice: the second copy 1, 2, 3 and 4 columns off a multiple of 4 from the first
    twice = []
    for i in range(4):
        s = 9_000 + 5_000 * i
        s2 = s + 20_000 + 4 * i + (i + 1)
        target[s2:s2 + mid] = target[s:s + mid]
        twice.append(s)
    reads = [_random(rng, ls[i % len(ls)]) for i in range(N_RANDOM[nwd])]
    planted = [_edit(rng, target[0:mid], 14, lo, hi)]
    for d in range(4):                                        # windows ending at T - 1 .. T - 4
        planted.append(_edit(rng, target[T - d - mid:T - d], 12 + d, lo, hi))
    for i, s in enumerate(twice):
        planted.append(_edit(rng, target[s:s + mid], 12 + i, lo, hi))
    ends = []
    for i in range(N_PLANTED - len(planted)):
        m = int(rng.integers(lo, hi + 1))
        s = int(rng.integers(64, T - m - 64)) // 4 * 4
        s += (i - (m - 1)) % 4                                # the window's last column is i mod 4
        ends.append(s + m - 1)
        planted.append(_edit(rng, target[s:s + m], 12 + i % 29, lo, hi))
    assert {e % 4 for e in ends} == {0, 1, 2, 3}
    assert len(planted) == N_PLANTED
    step = len(reads) // N_PLANTED
    for i, r in enumerate(planted):                           # spread through the batch rather than in a block of their own
        assert lo <= len(r) <= hi, len(r)
        reads.insert((step + 1) * i + 7, r)
    assert len(reads) == N_RANDOM[nwd] + N_PLANTED < 16384    # (the first level's threshold is fixed below 16,384 slots)
    assert {len(r) for r in reads} == set(ls)
    assert max(len(r) for r in reads) + DELAY_ROWS <= 32 * nwd
    n_open = open_reads(reads, target)
    assert n_open >= 4096, (nwd, n_open)
    return {"reads": reads, "target": target, "open": n_open, "planted": planted}


def mixed():
    b = PC.batch("A")
    assert {160 - len(r) for r in b["reads"]} == set(range(32))
    return b
