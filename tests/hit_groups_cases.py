"""Batches of tests/test_gpu_hit_groups.py, built the same way by the test and by its child process
(tests/hit_groups_child.py).  HW batches are distance, k = -1 against T = 70,001 symbols, as those of plain_column_cases, and
keep at least 4,096 uniform random reads open for the last level, which then takes the plain kernel: 17 segments of 4,128
columns (the test reads that from the library's debug line).

Planted reads: windows of the target with 12..40 edits (one word: 12..16 of its 32 rows; more would leave nothing of the
window), none in the last 8 rows, so that the window's last column is where the read ends.  The child asserts from the
reference's answers that the planted reads do end where they were put."""
import numpy as np

import plain_column_cases as PC

T = PC.T
SEG_LEN = 4128                       # of the main launch: roundup(ceil(T / 17), 16)
BOUNDARY = 3 * SEG_LEN               # first column of segment 3
HOMO = (20_000, 600)                 # start, length of the A-run in the target
DINUC = (30_000, 600)                # of the (AC)-run
N_RANDOM = {1: 7488, 5: 4096, 8: 4096}


def length(nwd):
    # 3 pad rows: the rows are bottom-aligned by a shift that is not 0.  One word: 31 rows, of which two thirds stay above the
    # first level's threshold of 8 against 70,001 random columns (plain_column_cases.batch_b); shorter reads resolve there.
    return 31 if nwd == 1 else 32 * nwd - 3


def _edits(nwd, i):
    return 12 + i % 5 if nwd == 1 else 12 + i % 29


def _edit_inside(rng, w, nedit):
    """substitutions, insertions and deletions in w[:-8]; the length stays"""
    head, tail = w[:-8].copy(), w[-8:]
    n0 = len(head)
    for _ in range(nedit):
        p = int(rng.integers(0, len(head)))
        kind = int(rng.integers(0, 3))
        if kind == 0 or len(head) <= 8:
            head[p] = PC._ACGT[(int(np.searchsorted(PC._ACGT, head[p])) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1 and len(head) > n0 - 4:
            head = np.delete(head, p)
        else:
            head = np.insert(head, p, PC._ACGT[rng.integers(0, 4)])
    # back to n0 rows at the front, where the window's end does not see it
    if len(head) > n0:
        head = head[len(head) - n0:]
    elif len(head) < n0:
        head = np.concatenate([PC._ACGT[rng.integers(0, 4, n0 - len(head))], head])
    return np.ascontiguousarray(np.concatenate([head, tail]))


def planted_ends(nwd):
    """last columns of the planted windows: every residue mod 4 and mod 16, the last column of a segment and the first of the
    next, and column T - 1 (the ragged-tail loop)"""
    ends = [9_000 + 16 * 7 * r + r for r in range(16)]          # residues 0..15 mod 16
    ends += [BOUNDARY - 1, BOUNDARY, BOUNDARY + 1, BOUNDARY - 2, T - 1, T - 2, T - 16, T - 17]
    return ends


def hw_batch(nwd):
    rng = np.random.default_rng(4300 + nwd)
    m = length(nwd)
    target = PC._random(rng, T)
    for start, n in (HOMO, DINUC):                                # 64 columns of G around the runs: no T next to them
        target[start - 64:start + n + 64] = PC._ACGT[2]
    target[HOMO[0]:HOMO[0] + HOMO[1]] = PC._ACGT[0]
    target[DINUC[0]:DINUC[0] + DINUC[1]] = np.tile(PC._ACGT[:2], DINUC[1] // 2)
    reads = [PC._random(rng, m) for _ in range(N_RANDOM[nwd])]
    planted, ends = [], planted_ends(nwd)
    for i, e in enumerate(ends):
        planted.append(_edit_inside(rng, target[e + 1 - m:e + 1], _edits(nwd, i)))
    # tandem repeats: a read of the run with substitutions that the run cannot match scores the same in every column of the
    # run that holds it (homopolymer: hundreds of end locations in neighbouring columns, far more than a slot's 16 and a
    # segment's 16) or in every second one (dinucleotide: the score moves by one between neighbours); on the way in the score
    # improves column after column.
    nsub = 9 if nwd == 1 else 14                                  # (above the first level's threshold of 8)
    for run, unit in ((HOMO, PC._ACGT[:1]), (DINUC, PC._ACGT[:2])):
        r = np.tile(unit, m // len(unit) + 1)[:m].copy()
        at = rng.choice(m - 8, size=nsub, replace=False)
        r[at] = PC._ACGT[3]                                       # T: in neither run
        planted.append(np.ascontiguousarray(r))
    first_planted = 7
    for i, r in enumerate(planted):                               # spread through the batch, not a block of their own
        reads.insert(first_planted + 65 * i, r)
    where = [first_planted + 65 * i for i in range(len(planted))]
    return {"reads": reads, "target": target, "mode": "HW", "planted": where, "ends": ends, "nwd": nwd}


def shw_batch():
    """a small SHW batch of five-word reads: prefixes of the target with a few edits (hits in the first columns), random
    reads, and a read of the target's first symbol only"""
    rng = np.random.default_rng(4390)
    m = length(5)
    target = PC._random(rng, T)
    target[:40] = PC._ACGT[2]                                      # a run at the start: ties in neighbouring columns
    reads = []
    for i in range(192):
        if i % 3 == 0:
            reads.append(PC._random(rng, m - i % 29))
        else:
            mm = m - i % 29                                        # 129..157 rows: one group of five words
            reads.append(_edit_inside(rng, target[:mm], i % 14))
    reads.append(np.ascontiguousarray(target[:m]))
    return {"reads": reads, "target": target, "mode": "SHW", "nwd": 5}


NAMES = ["W1", "W5", "W8", "SHW"]


def batch(name):
    if name == "SHW":
        return shw_batch()
    return hw_batch(int(name[1:]))
