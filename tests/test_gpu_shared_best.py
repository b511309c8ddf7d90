"""The dense last level of HW read batches with one running best per read shared by its segments (ReadScanArgs::liveBest,
scan_reads_kernel<NWD, 2, true> and <NWD, 2, true, true>).  A segment starts from what the others have found,
publishes what it finds and looks again every kLivePeriod columns, so WHEN a segment learns of a bound depends on how the
waves happen to run; the results must not.  tests/shared_best_cases.py plants the reads for which it could matter (the
minimum only in the last segment, a tie across an imported bound, a strictly better window after segment 0's, more than 16
equal hits in one segment and over several, a hit in the ragged tail) in batches of 1, 2, 5 and 8 words on both row forms.
A child process runs each batch twice, requires identical output and compares every field of every read with the reference;
the library's own EDLIB_AMD_DEBUG lines must say that the last level took the plain kernel with at least 4,096 slots, on the
expected rows, in the 17 segments of 4,128 columns that the planted windows are placed by.
(These batches reach the last level through the banded first pass: the exact seed filter takes groups from 2^30
read-columns on, sixteen times this size, and hands the same open reads to the same last level.)
The shapes of the planted reads are checked with the reference alone, without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shared_best_cases as SC
from test_gpu_delay_rows import _SCAN_ROWS
from test_gpu_plain_column import _LEVEL_LINE

CASES = [(nwd, form) for nwd in SC.WORDS for form in SC.FORMS]


def _reference(reads, target):
    from oracle import oracle as O
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    ref = O.pool_align(np.concatenate(reads), qoff, target, np.array([0, len(target)], dtype=np.int64), True, "HW", "distance", -1)
    ends = [[int(e) for e in ref["ends"][ref["locOff"][i]:ref["locOff"][i + 1]]] for i in range(len(reads))]
    return [int(d) for d in ref["editDistance"]], ends


@pytest.mark.parametrize("nwd,form", CASES)
def test_lengths_pick_the_row_form_and_leave_the_plain_kernel_its_slots(nwd, form):
    b = SC.batch(nwd, form, True)
    assert 4096 <= b["open"] <= len(b["reads"]) < 16384
    longest = max(len(r) for r in b["reads"])
    assert len({len(r) for r in b["reads"]}) == 2 and (longest + 31) // 32 == nwd
    assert (longest + 3 <= 32 * nwd) == (form == "delay")
    assert SC.T >= 16 * 4096 and SC.SEGMENTS * SC.SEG_LEN >= SC.T > (SC.SEGMENTS - 1) * SC.SEG_LEN and SC.T % 16 == 1


@pytest.mark.parametrize("nwd,form", [c for c in CASES if c[0] > 1])
def test_planted_reads_are_what_they_say(nwd, form):
    b = SC.batch(nwd, form)
    names = list(SC.PLANTS)
    reads = [b["reads"][b["where"][n]] for n in names]
    dist, ends = _reference(reads, b["target"])
    dist, ends = dict(zip(names, dist)), dict(zip(names, ends))
    last = SC.SEGMENTS - 1
    E = SC.edits(nwd)
    assert all(8 < dist[n] <= E for n in names), dist                    # open after the first level (threshold 8)
    assert {SC.segment_of(e) for e in ends["a"]} == {last} and max(ends["a"]) < SC.T - 1
    assert {SC.segment_of(e) for e in ends["b"]} == {0, last}
    d0, _ = _reference([reads[names.index("c")]], b["target"][:SC.SEG_LEN])
    assert dist["c"] < d0[0] <= E + 5 and {SC.segment_of(e) for e in ends["c"]} == {9}
    assert len(ends["d1"]) > 16 and {SC.segment_of(e) for e in ends["d1"]} == {7}
    per = [sum(SC.segment_of(e) == s for e in ends["d2"]) for s in range(SC.SEGMENTS)]
    assert sum(per) > 16 and max(per) <= 16 and sum(p > 0 for p in per) == 3, per
    assert ends["e"][-1] == SC.T - 1 and SC.T - 1 >= SC.T // 16 * 16     # a column of the ragged tail


@pytest.mark.gpu
@pytest.mark.parametrize("nwd,form", CASES)
def test_two_runs_agree_with_each_other_and_with_the_reference(nwd, form):
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "shared_best_child.py"),
                        str(nwd), form], capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    levels = [(int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(p.stderr)]
    scans = [tuple(int(x) for x in m.groups()[:4]) + (m.group(5),) for m in _SCAN_ROWS.finditer(p.stderr)]
    print(nwd, form, levels, scans)
    assert len(levels) == 2 and levels[0] == levels[1], levels           # two runs, one level after the first pass each
    n, plain = levels[0]
    assert plain == 1 and n >= 4096, levels
    # (where every read stays open the first pass has as many lanes, on rows built from the top)
    main = [s for s in scans if s[0] == nwd and s[1] == n and s[2] > 1 and s[4] != "top"]
    assert len(main) == 2, scans
    assert all(s[2:] == (SC.SEGMENTS, SC.SEG_LEN, form) for s in main), scans
    assert [s for s in scans if s[0] == nwd and s[1] == n and s[2:4] == (1, 4096) and s[4] == form], scans   # the pre-scan
