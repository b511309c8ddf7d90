"""Batches of tests/test_gpu_shared_best.py, built the same way by the test and by its child process
(tests/shared_best_child.py): the dense last level of HW read batches with one running best per read shared by its segments
(ReadScanArgs::liveBest).  HW, distance, k = -1, against T = 70,001 symbols as tests/plain_column_cases.py: the
smallest target with a 4,096-column pre-scan (T >= 16 x 4,096), and at 4,096 to 16,383 open reads the last level cuts it into
17 segments of 4,128 columns, four looks at the shared best each, the last one ending in a ragged tail of one column.

One batch per word count (1, 2, 5, 8) and row form:
  "delay"   reads of 32 nwd - 3 and 32 nwd - 7 symbols (one word: 29 and 27): the longest leaves the three delay rows their
            room, scan_reads_kernel<NWD, 2, true, true>;
  "bottom"  reads of 32 nwd and 32 nwd - 2 symbols: no room for delay rows, scan_reads_kernel<NWD, 2, true>.
(Seven delay rows, for which 32 nwd - 7 would be the longest eligible length, are not built; those reads ride along.)

Planted reads, each the longest length of its batch, windows with E substitutions (12; one word: 10), spread through the batch:
  a   the window stands only in the last segment;
  b   the same window in the first and in the last segment: a tie across a bound the last segment imports;
  c   a copy with E + 5 substitutions in segment 0 (the pre-scan finds it) and the window itself, strictly better, in segment 9;
  d1  a stretch of period 8 inside segment 7: 25 equal hits eight columns apart, more than a segment's 16 positions;
  d2  a motif standing six times in each of the segments 3, 5 and 12: 18 equal hits, every segment within its 16 positions;
  e   the window ends at column T - 1, the ragged tail.
At one word a random 29-mer is already within 9 or 10 edits of some window of the target, so there the planted reads tie or lose
against the background; what they are then is whatever the reference says, and only the larger word counts assert the shapes.

`batch(..., count_open=True)` counts with the reference the reads above the first level's threshold: the last level takes
the plain kernel only with at least 4,096 of them."""
import functools

import numpy as np

from delay_rows_model import dp_bottom_row
from pair_shift_cases import open_reads
from plain_column_cases import T, _ACGT, _random

WORDS = (1, 2, 5, 8)
FORMS = ("delay", "bottom")
SEGMENTS, SEG_LEN = 17, 4128
N_RANDOM = {(1, "delay"): 12000, (1, "bottom"): 9000}
PLANTS = ("a", "b", "c", "d1", "d2", "e")


def lengths(nwd, form):
    if form == "bottom":
        return [32 * nwd, 32 * nwd - 2]
    return [29, 27] if nwd == 1 else [32 * nwd - 3, 32 * nwd - 7]


def edits(nwd):
    return 10 if nwd == 1 else 12


def _subs(rng, w, n):
    w = w.copy()
    for p in rng.choice(len(w), n, replace=False):
        w[p] = _ACGT[(int(np.searchsorted(_ACGT, w[p])) + 1 + int(rng.integers(0, 3))) % 4]
    return np.ascontiguousarray(w)


def segment_of(col):
    return int(col) // SEG_LEN


@functools.lru_cache(maxsize=None)
def batch(nwd, form, count_open=False):
    assert nwd in WORDS and form in FORMS
    rng = np.random.default_rng(4500 + 10 * nwd + FORMS.index(form))
    ls = lengths(nwd, form)
    L, E = ls[0], edits(nwd)
    target = _random(rng, T)
    planted = {}
    planted["a"] = _subs(rng, target[68200:68200 + L], E)
    target[67000:67000 + L] = target[1000:1000 + L]
    planted["b"] = _subs(rng, target[1000:1000 + L], E)
    planted["c"] = _subs(rng, target[40000:40000 + L], E)
    target[2000:2000 + L] = _subs(rng, planted["c"], E + 5)
    unit = np.array([0, 1, 3, 2, 2, 0, 3, 1], dtype=np.int64)[rng.permutation(8)]
    span = L + 8 * 24
    target[30000:30000 + span] = _ACGT[np.resize(unit, span)]
    for _ in range(16):                                                     # (substitutions near an end can do one better
        planted["d1"] = _subs(rng, target[30000:30000 + L], E)             # against the random columns beside the stretch)
        row = dp_bottom_row([int(np.searchsorted(_ACGT, x)) for x in planted["d1"]],
                            np.searchsorted(_ACGT, target[29700:30000 + span + 300]))
        if np.count_nonzero(row == row.min()) == 25 and row.min() == E:
            break
    else:
        raise AssertionError("no read ties along the whole stretch")
    motif = _random(rng, L)
    for base in (12500, 20800, 49700):
        for i in range(6):
            target[base + 600 * i:base + 600 * i + L] = motif
    planted["d2"] = _subs(rng, motif, E)
    planted["e"] = _subs(rng, target[T - L:T], E)
    n_random = N_RANDOM.get((nwd, form), 4200)
    reads = [_random(rng, ls[i % 4 == 3]) for i in range(n_random)]        # three of the longer length, one of the shorter
    where = {}
    for i, name in enumerate(PLANTS):                                       # different waves, different lanes
        at = 200 + 611 * i
        reads.insert(at, planted[name])
        where[name] = at
    for name, at in where.items():
        assert reads[at] is planted[name]
    assert {len(r) for r in reads} == set(ls) and len(reads) < 16384        # (the first level's threshold is fixed below 16,384 slots)
    out = {"reads": reads, "target": target, "where": where, "length": L}
    if count_open:
        out["open"] = open_reads(reads, target)
        assert out["open"] >= 4096, (nwd, form, out["open"])
    return out
