"""-m gpu: the group hit test of scan_reads_kernel (one test per four columns, the per-column test only for lanes that pass
it).

HW batches of 1, 5 and 8 words (tests/hit_groups_cases.py) plant windows that end in columns of every residue mod 16, in the
last column of a segment and the first of the next, in column T - 1 (the ragged-tail loop), and reads of tandem repeats whose
score ties in neighbouring columns hundreds of times.  A small SHW batch goes through scan_reads_kernel<5, 1>.  Every field of
every read is compared with the reference in a child process (EDLIB_AMD_DEBUG is read when the library loads), and the
library's own debug lines must say that the kernel under test ran: the last level took the plain kernel with at least 4,096
slots, in segments of the length the planted boundary windows assume."""
import os
import re
import subprocess
import sys

import pytest

import hit_groups_cases as HC

pytestmark = pytest.mark.gpu

_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned \(plain=(\d)\)")
_SCAN_LINE = re.compile(r"scanGroup nwords=(\d+) mode=(\d) nlanes=(\d+) S=(\d+) segLen=(\d+) ")


def _run(name):
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hit_groups_child.py"), name],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    levels = [(int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(p.stderr)]
    scans = [tuple(int(x) for x in m.groups()) for m in _SCAN_LINE.finditer(p.stderr)]
    print(name, levels, scans)
    return levels, scans


def _main_launch_of_plain_last_level(levels, scans, nwd):
    """(nlanes, S, segLen) of the segmented launch of the last level, which must be on the plain kernel"""
    assert levels, "no level after the first pass"
    n, plain = levels[-1]
    assert plain == 1 and n >= 4096, levels
    mine = [s for s in scans if s[0] == nwd and s[1] == 2 and s[2] == n]
    assert [s for s in mine if s[3] == 1 and s[4] == 4096], scans            # the pre-scan of the first 4,096 columns
    main = [s for s in mine if s[3] > 1]
    assert main, scans
    _, _, nlanes, S, seg_len = main[-1]
    assert S * seg_len >= HC.T > (S - 1) * seg_len and HC.T % 16 != 0 and seg_len % 16 == 0      # the ragged tail is there
    return nlanes, S, seg_len


@pytest.mark.parametrize("nwd", [1, 5, 8])
def test_planted_windows_and_repeats(nwd):
    levels, scans = _run("W%d" % nwd)
    nlanes, S, seg_len = _main_launch_of_plain_last_level(levels, scans, nwd)
    assert seg_len == HC.SEG_LEN, (S, seg_len)                               # where the boundary windows were planted


def test_small_shw_batch_on_the_plain_kernel():
    levels, scans = _run("SHW")
    assert not levels
    # mode 1 has no banded kernel: scanGroup sends it to scan_reads_kernel<5, 1>, one segment of the columns SHW can reach
    assert scans and all(s[0] == 5 and s[1] == 1 and s[3] == 1 for s in scans), scans
