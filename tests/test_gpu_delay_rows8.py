"""The plain full-height HW kernel on rows built with seven delay rows (scan_reads_kernel<NWD, 2, true, 7>, reads_column_asm.hpp,
DESIGN.md 3): the score moves once per eight columns, from the top bytes of the last word's Ph / Mh, and the hit test runs
once per eight.  One batch per word count 1, 2, 5, 8 whose longest read leaves exactly seven rows free (pads 7 .. 31), and
beside each one whose longest read leaves six: that one must keep the three-row form.  tests/delay_rows8_cases.py has what
is planted and why every read is unrelated enough to reach the last level.  Every field of every read is compared with the
reference in a child process, twice on one resident batch; the library's own EDLIB_AMD_DEBUG lines must say that the last
level took the plain kernel with at least 4,096 slots, a pre-scan and a main launch of several segments of 4,128 columns ending
in the ragged tail, on delay rows of the expected depth.  What the batches hold is checked with the reference without a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import delay_rows8_cases as DC
from test_gpu_plain_column import _LEVEL_LINE, _reached_plain_kernel

# the scan line and, where the rows carry delay rows, the depth on the line directly after it
_SCAN = re.compile(r"scanGroup nwords=(\d+) mode=2 nlanes=(\d+) S=(\d+) segLen=(\d+) [^\n]*? rows=(\w+) kernel=(\w+) syms=4\n"
                   r"(?:\[edlib_amd\] scanGroup delayRows=(\d+)\n)?")


_REF = {}


def _planted_reference(name):
    """the reference's answers for the planted reads of a batch (once per batch)"""
    if name not in _REF:
        from oracle import oracle as O
        b = DC.batch(name)
        reads = [r for _, r, _ in b["planted"]]
        qoff = np.zeros(len(reads) + 1, dtype=np.int64)
        qoff[1:] = np.cumsum([len(r) for r in reads])
        ref = O.pool_align(np.concatenate(reads), qoff, b["target"], np.array([0, DC.T], dtype=np.int64), True, "HW", "distance", -1)
        _REF[name] = [(int(ref["editDistance"][i]), [int(e) for e in ref["ends"][ref["locOff"][i]:ref["locOff"][i + 1]]])
                      for i in range(len(reads))]
    return _REF[name]


@pytest.mark.parametrize("name", DC.NAMES)
def test_cases_hold_the_pads_and_leave_the_plain_kernel_its_slots(name):
    b = DC.batch(name)                                      # asserts lengths, count and the reads left open (reference, CPU)
    nwd, free = DC.words(name), DC.free_rows(name)
    assert 4096 <= b["open"] <= len(b["reads"]) < 8192
    pads = {32 * nwd - len(r) for r in b["reads"]}
    assert min(pads) == free and set(range(free, 32)) <= pads
    assert sum(1 for r in b["reads"] if 32 * nwd - len(r) == free) >= 64


@pytest.mark.parametrize("name", DC.NAMES)
def test_planted_reads_are_what_they_are_meant_to_be(name):
    """by the reference: every planted read is above the first level's threshold and ends where it was planted; the ends cover
    the columns 0 .. 7 and T - 8 .. T - 1, every residue mod 8, both sides of three segment boundaries, two columns of one
    group, twenty columns of one segment, and the liveBest reads score best in the far segment only"""
    b = DC.batch(name)
    ref = _planted_reference(name)
    kinds = {}
    for (kind, read, e), (dist, ends) in zip(b["planted"], ref):
        assert dist > 8, (kind, dist)
        assert e in ends, (kind, e, dist, ends[:20])
        kinds.setdefault(kind, []).append((e, dist, ends, read))
    assert {e for e, _, _, _ in kinds["head"]} == set(range(8))
    assert {e for e, _, _, _ in kinds["tail"]} == set(range(DC.T - 8, DC.T))
    assert {e % 8 for e, _, _, _ in kinds["group"]} == set(range(8))
    seams = {e for e, _, _, _ in kinds["seam"]}
    for bnd in (1, 2, 9):
        assert {bnd * DC.SEG - 1, bnd * DC.SEG, bnd * DC.SEG + 1, bnd * DC.SEG + 4} <= seams
    for e, _, ends, _ in kinds["pair"]:
        assert e - 1 in ends and (e - 1) // 8 == e // 8, (e, ends)
    (e, dist, ends, _), = kinds["twenty"]
    assert set(b["twenty_ends"]) <= set(ends) and len(ends) >= 20
    assert len({x // DC.SEG for x in b["twenty_ends"]}) == 1
    for e, dist, ends, read in kinds["live"]:
        assert {x // DC.SEG for x in ends} == {e // DC.SEG}, (e, ends)     # the worse copy's segment holds no best end
    # a junk copy comes down by 1 per column into its hit: the model's textbook DP on one of them
    import delay_rows8_model as M
    e, dist, ends, read = kinds["group"][0]
    sym = {65: 0, 67: 1, 71: 2, 84: 3, 78: 4}
    lo = e - 2 * len(read)
    row = M.dp_bottom_row([sym[int(x)] for x in read], [sym[int(x)] for x in b["target"][lo:e + 1]])
    # (a whole group's worth; a read of one word hovers too close above its best for more than six)
    n = 6 if DC.words(name) == 1 else 8
    assert [int(x) - dist for x in row[-n:]] == list(range(n - 1, -1, -1)), row[-n:]


def _run(name):
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "delay_rows8_child.py"), name],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    assert p.stderr.count("[child] run") == 2
    runs = p.stderr.split("[child] run 1 compared\n")
    assert len(runs) == 2
    out = []
    for text in runs:
        levels = [(int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(text)]
        scans = [tuple(int(x) for x in m.groups()[:4]) + (m.group(5), m.group(6), int(m.group(7) or 0)) for m in _SCAN.finditer(text)]
        print(name, levels, scans)
        out.append((levels, scans))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", DC.NAMES)
def test_every_field_twice_on_rows_of_the_expected_depth(name):
    nwd, depth = DC.words(name), DC.expected_depth(name)
    for levels, scans in _run(name):                       # the first run and the one that reuses the level's records
        _reached_plain_kernel(levels, [s[:4] for s in scans], nwd)
        assert levels[0][0] >= DC.batch(name)["open"]       # padding slots of the rebuilt rows may add to the count
        # the launches over all lanes of the last level: the pre-scan and the main launch
        mine = [s for s in scans if s[0] == nwd and s[1] == levels[0][0]][-2:]
        assert len(mine) == 2 and mine[0][2:4] == (1, 4096) and mine[1][2] > 1, scans
        assert mine[1][3] == DC.SEG, scans                  # the boundaries that the planted windows stand at
        for s in mine:
            assert s[4:] == ("delay", "plain", depth), scans
        # nothing else reads such rows, and every line that names delay rows names their depth
        assert [s[4] for s in scans].count("delay") == 2 and "bottom" not in {s[4] for s in scans}, scans
        assert all((s[6] > 0) == (s[4] == "delay") for s in scans), scans
