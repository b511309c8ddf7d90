"""The bottom-aligned full-height column with `<< 1` on register pairs (scan_reads_kernel<NWD, 2, true>, reads_column_asm.hpp,
DESIGN.md 3) at every word count but five, which batch A of test_gpu_plain_column.py covers at every pad: reads at every pad
of the word count and planted windows at both ends of the target (tests/pair_shift_cases.py).  Every field of every read is
compared with the reference in a child process, and the library's own EDLIB_AMD_DEBUG lines must say that the last level took
the plain kernel with at least 4,096 slots and a main launch of several segments -- the smallest shape at which this kernel
runs at all.  The builder's count of reads left open by the first level is checked without a GPU."""
import os
import subprocess
import sys

import pytest

import pair_shift_cases as PS
from test_gpu_plain_column import _LEVEL_LINE, _SCAN_LINE, _reached_plain_kernel


@pytest.mark.parametrize("nwd", PS.WORDS)
def test_cases_leave_the_plain_kernel_its_slots(nwd):
    b = PS.batch(nwd)                                       # asserts lengths, count and the reads left open (reference, CPU)
    assert 4096 <= b["open"] <= len(b["reads"]) <= 4700
    assert {32 * nwd - len(r) for r in b["reads"]} == set(range(17 if nwd == 2 else 32))
    assert b["reads"][7].tobytes() != b["target"][:len(b["reads"][7])].tobytes()        # planted, edited


def _run(nwd):
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pair_shift_child.py"), str(nwd)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    levels = [(int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(p.stderr)]
    scans = [tuple(int(x) for x in m.groups()) for m in _SCAN_LINE.finditer(p.stderr)]
    print(nwd, levels, scans)
    return levels, scans


@pytest.mark.gpu
@pytest.mark.parametrize("nwd", PS.WORDS)
def test_every_pad_and_planted_windows(nwd):
    levels, scans = _run(nwd)
    _reached_plain_kernel(levels, scans, nwd)
    assert levels[0][0] >= PS.batch(nwd)["open"]            # padding slots of the rebuilt rows may add to the count
