"""The plain full-height HW kernel on rows built with delay rows (scan_reads_kernel<NWD, 2, true, true>, reads_column_asm.hpp,
DESIGN.md 3): the score moves once per four columns, from the top nibbles of the last word's Ph / Mh.  One batch per word
count with every read short enough for the three delay rows (tests/delay_rows_cases.py: pads 3..31, planted windows at both
ends of the target, ending at every residue mod 4, and standing twice), every field of every read compared with the reference
in a child process; the library's own EDLIB_AMD_DEBUG lines must say that the last level took the plain kernel with at least
4,096 slots, a pre-scan and a main launch of several segments ending in the ragged tail, all on delay rows.  A five-word batch
with reads at every pad 0..31 is not eligible: it must name the bottom-aligned rows without delay rows and still match.
The builder's own counts are checked without a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import delay_rows_cases as DR
from test_gpu_plain_column import _LEVEL_LINE, _reached_plain_kernel

_SCAN_ROWS = re.compile(r"scanGroup nwords=(\d+) mode=2 nlanes=(\d+) S=(\d+) segLen=(\d+) .*? rows=(\w+)")


@pytest.mark.parametrize("nwd", DR.WORDS)
def test_cases_fit_the_delay_rows_and_leave_the_plain_kernel_its_slots(nwd):
    b = DR.batch(nwd)                                       # asserts lengths, count and the reads left open (reference, CPU)
    assert 4096 <= b["open"] <= len(b["reads"]) < 16384
    pads = {32 * nwd - len(r) for r in b["reads"]}
    assert min(pads) == 3 and max(pads) <= 31 and pads == set(range(3, max(pads) + 1))
    assert b["reads"][7].tobytes() != b["target"][:len(b["reads"][7])].tobytes()        # planted, edited


def test_planted_reads_end_at_every_residue_and_tie_across_groups():
    """by the reference: the planted reads' end locations cover every column mod 4, the last four columns of the target, and at
    least one read has best ends in two different groups of four columns at different places in them"""
    from oracle import oracle as O
    b = DR.batch(5)
    reads, target = b["planted"], b["target"]
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    ref = O.pool_align(np.concatenate(reads), qoff, target, np.array([0, len(target)], dtype=np.int64), True, "HW", "distance", -1)
    ends = [np.asarray(ref["ends"][ref["locOff"][i]:ref["locOff"][i + 1]]) for i in range(len(reads))]
    allends = np.concatenate(ends)
    assert {int(e) % 4 for e in allends} == {0, 1, 2, 3}
    assert {DR.T - 1, DR.T - 2, DR.T - 3, DR.T - 4} <= {int(e) for e in allends}
    assert any(len(e) >= 2 and e[-1] // 4 != e[0] // 4 and e[-1] % 4 != e[0] % 4 for e in ends)


def _run(name):
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "delay_rows_child.py"), str(name)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    levels = [(int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(p.stderr)]
    scans = [tuple(int(x) for x in m.groups()[:4]) + (m.group(5),) for m in _SCAN_ROWS.finditer(p.stderr)]
    print(name, levels, scans)
    return levels, scans


def _rows_of_last_level(levels, scans, nwd):
    """the form of the launches over all lanes of the last level: the pre-scan and the main launch"""
    _reached_plain_kernel(levels, [s[:4] for s in scans], nwd)
    # (where every read stays open the first pass has as many lanes: the level's own launches are the last two)
    mine = [s for s in scans if s[0] == nwd and s[1] == levels[0][0]][-2:]
    assert len(mine) == 2 and mine[0][2:4] == (1, 4096) and mine[1][2] > 1, scans
    return {s[4] for s in mine}


@pytest.mark.gpu
@pytest.mark.parametrize("nwd", DR.WORDS)
def test_every_eligible_pad_and_planted_windows(nwd):
    levels, scans = _run(nwd)
    assert _rows_of_last_level(levels, scans, nwd) == {"delay"}, scans
    assert levels[0][0] >= DR.batch(nwd)["open"]            # padding slots of the rebuilt rows may add to the count
    assert [s[4] for s in scans].count("delay") == 2 and "bottom" not in {s[4] for s in scans}, scans   # nothing else reads such rows


@pytest.mark.gpu
def test_reads_at_every_pad_keep_the_rows_without_delay():
    levels, scans = _run("mixed")
    assert _rows_of_last_level(levels, scans, 5) == {"bottom"}, scans
