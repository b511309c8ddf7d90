"""-m gpu: the plain full-height column on bottom-aligned rows (scan_reads_kernel<NWD, 2, true>): the last level
of HW read batches whose leftovers are unrelated sequence.  Every field of every read is compared with the reference (_check
of test_gpu_long_reads, in a child process), and the library's own EDLIB_AMD_DEBUG line must say that the last level took the
plain kernel with at least 4,096 slots -- below that the level stays on the banded kernel and the test would check nothing
new.  The batches (tests/plain_column_cases.py) are the smallest that go through the 4,096-column pre-scan, the segmented
main launch and the ragged-tail loop."""
import os
import re
import subprocess
import sys

import pytest

import plain_column_cases as PC

pytestmark = pytest.mark.gpu

_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned \(plain=(\d)\)")
_SCAN_LINE = re.compile(r"scanGroup nwords=(\d+) mode=2 nlanes=(\d+) S=(\d+) segLen=(\d+) ")


def _run(name):
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "plain_column_child.py"), name],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    levels = [(int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(p.stderr)]
    scans = [tuple(int(x) for x in m.groups()) for m in _SCAN_LINE.finditer(p.stderr)]
    print(name, levels, scans)
    return levels, scans


def _reached_plain_kernel(levels, scans, nwd):
    assert len(levels) == 1, levels                         # one group, one level after the first pass: the last one
    n, plain = levels[0]
    assert plain == 1 and n >= 4096, levels
    # the two launches of that level over all its lanes: the pre-scan (one segment of 4,096 columns) and the main launch
    # (several segments, the last one ending at T = 70,001: the ragged tail)
    mine = [s for s in scans if s[0] == nwd and s[1] == n]
    assert [s for s in mine if s[2] == 1 and s[3] == 4096], scans
    main = [s for s in mine if s[2] > 1]
    assert main and main[-1][2] * main[-1][3] >= PC.T > (main[-1][2] - 1) * main[-1][3] and PC.T % 16 != 0, scans


def test_batch_a_every_pad_and_planted_windows():
    b = PC.batch("A")
    assert {160 - len(r) for r in b["reads"]} == set(range(32))
    levels, scans = _run("A")
    _reached_plain_kernel(levels, scans, 5)


@pytest.mark.parametrize("nwd", range(1, 9))
def test_batch_b_every_word_count(nwd):
    b = PC.batch("B%d" % nwd)
    assert {len(r) for r in b["reads"]} == {32 * nwd - 20, 32 * nwd - 1, 32 * nwd} and len(b["reads"]) == PC.N_READS_B[nwd] >= 4160
    levels, scans = _run("B%d" % nwd)
    _reached_plain_kernel(levels, scans, nwd)
