"""-m gpu: HW read scans over shared targets of exactly 8 and 16 symbols (Peq rows [word][8 | 16 symbols][lane] in LDS,
DESIGN.md 3) at every word count, and the long word groups of the full-height kernel:
  scan_reads_full_kernel<N, 8|16>, N = 1..8: the last level of a batch that leaves at least 4,096 unrelated reads open, with
      the 4,096-column pre-scan, a main launch of several segments that ends in the masked last block (T = 70,001), planted
      windows at column 0 and at T - 1 .. T - 4, a read with 20 end locations (the exact pass) and, once per layout, a fixed k;
  scan_reads_full_kernel<10|12, 4|8>: the same for reads of 257..384 bases (16 symbols: the piece filter takes those);
  scan_reads_full_kernel<14|16, 8>: what the piece filter hands back (Batch::runLongReads);
  scan_reads_banded_kernel<N, 8|16>, N = 1..8: small batches of reads at distances from 0 to unrelated, every band height.
Every field of every read is compared with the reference in a child process (_check of test_gpu_long_reads; the batches:
tests/wide_rows_cases.py, checked without a GPU by tests/test_wide_rows_cases.py), and the library's own EDLIB_AMD_DEBUG lines
must name the kernel of every launch the test is about (scanGroup ... kernel=full|banded|plain syms=): were the routing to
change, these tests would otherwise pass while checking nothing new."""
import json
import os
import re
import subprocess
import sys

import pytest

import wide_rows_cases as WR
from wide_rows_cases import T

pytestmark = pytest.mark.gpu

_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned \(plain=(\d)\)")
_SCAN_LINE = re.compile(r"scanGroup nwords=(\d+) mode=2 nlanes=(\d+) S=(\d+) segLen=(\d+) .* rows=(\w+) kernel=(\w+) syms=(\d+)$")
_FIELDS = ("nwords", "nlanes", "S", "segLen", "rows", "kernel", "syms")


def _run(name):
    """the child's statistics and the library's lines in the order they were written: ("scan", {...}) / ("level", n, plain)"""
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_rows_child.py"), name],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("stats ")][-1][6:])
    events = []
    for ln in p.stderr.splitlines():
        m = _SCAN_LINE.search(ln)
        if m:
            events.append(("scan", {f: (v if f in ("rows", "kernel") else int(v)) for f, v in zip(_FIELDS, m.groups())}))
        m = _LEVEL_LINE.search(ln)
        if m:
            events.append(("level", int(m.group(2)), int(m.group(3))))
    assert sum(1 for ln in p.stderr.splitlines() if "scanGroup nwords=" in ln) == sum(1 for e in events if e[0] == "scan")
    print(name, st, [e if e[0] == "level" else tuple(e[1].values()) for e in events])
    return st, events


def _reached_full_kernel(st, events, nwd, syms, n_open):
    levels = [e for e in events if e[0] == "level"]
    assert len(levels) == 1, levels                         # one group, one level after the first pass: the last one
    _, n, plain = levels[0]
    assert plain == 1 and n >= 4096 and n >= n_open, levels  # (padding slots of the rebuilt rows may add to the count)
    # the level's launches, in order: the 64-lane sample on the banded kernel, then over all n lanes the pre-scan (one segment
    # of 4,096 columns) and the main launch (several segments, the last one ending at T = 70,001: the masked last block)
    at = events.index(levels[0])
    assert at >= 3 and all(e[0] == "scan" for e in events[at - 3:at]), events[:at]
    sample, pre, main = (e[1] for e in events[at - 3:at])
    assert sample["nlanes"] == 64 and sample["kernel"] == "banded" and sample["syms"] == syms, sample
    for s in (pre, main):
        assert (s["nwords"], s["nlanes"], s["kernel"], s["syms"], s["rows"]) == (nwd, n, "full", syms, "top"), s
    assert pre["S"] == 1 and pre["segLen"] == 4096, pre
    assert main["S"] > 1 and main["S"] * main["segLen"] >= T > (main["S"] - 1) * main["segLen"] and T % 16 != 0, main
    # everything else (the first pass, the exact pass) stays on the banded kernel
    assert all(e[1]["kernel"] == "banded" and e[1]["syms"] == syms for e in events[:at - 2] + events[at + 1:] if e[0] == "scan")
    assert st["path"] & 1
    assert st["overflow_units"] >= 1                        # the read with 20 end locations went through the exact pass


@pytest.mark.parametrize("layout", WR.LAYOUTS)
@pytest.mark.parametrize("nwd", WR.WORDS_FULL)
def test_full_height_every_word_count(nwd, layout):
    st, events = _run("full:%d:%s:distance:-1" % (nwd, layout))
    _reached_full_kernel(st, events, nwd, WR.SYMS[layout], WR.full(nwd, layout)["open"])


@pytest.mark.parametrize("nwd,layout", WR.LOCATIONS_RUNS)
def test_full_height_locations_with_fixed_k(nwd, layout):
    """the same batch with start locations asked for and k = 40: thresholds min(k, m), reads above k report nothing"""
    st, events = _run("full:%d:%s:locations:%d" % (nwd, layout, WR.K_LOCATIONS))
    _reached_full_kernel(st, events, nwd, WR.SYMS[layout], WR.full(nwd, layout)["open"])


@pytest.mark.parametrize("layout", ["base", "rows8"])
@pytest.mark.parametrize("nwd", WR.WORDS_LONG)
def test_full_height_ten_and_twelve_words(nwd, layout):
    """reads of 257..320 / 321..384 bases that stay on the lanes, on 4 and on 8 rows"""
    st, events = _run("full:%d:%s:distance:-1" % (nwd, layout))
    _reached_full_kernel(st, events, nwd, WR.SYMS[layout], WR.full(nwd, layout)["open"])
    assert not st["path"] & 4


def test_sixteen_rows_send_257_to_384_bases_through_the_piece_filter():
    """no 10- / 12-word group on 16 rows (64 KB of LDS rows per wave): same answers by another route"""
    st, events = _run("long16:0:rows16:distance:-1")
    assert st["path"] & 4
    assert not [e for e in events if e[0] == "scan" and e[1]["nwords"] > 8], events


def test_handed_back_to_fourteen_and_sixteen_words_on_eight_rows():
    """385..512 bases against 8 symbols: the piece filter hands the unrelated reads back to the full-height kernel"""
    st, events = _run("back:0:rows8:distance:-1")
    assert st["path"] & 4 and st["path"] & 1
    scans = [e[1] for e in events if e[0] == "scan"]
    for nwd in (14, 16):
        mine = [s for s in scans if s["nwords"] == nwd and s["kernel"] == "full"]
        assert mine and all(s["syms"] == 8 and s["nlanes"] >= 100 for s in mine), scans


def _stayed_on_banded_kernel(st, events, nwd, syms):
    scans = [e[1] for e in events if e[0] == "scan"]
    levels = [e for e in events if e[0] == "level"]
    assert len(scans) >= 2 and all((s["nwords"], s["kernel"], s["syms"]) == (nwd, "banded", syms) for s in scans), scans
    assert levels and all(plain == 0 and n < 4096 for _, n, plain in levels), levels
    assert st["path"] & 1


@pytest.mark.parametrize("layout", WR.LAYOUTS)
@pytest.mark.parametrize("nwd", WR.WORDS_FULL)
def test_banded_every_band_height(nwd, layout):
    st, events = _run("banded:%d:%s:distance:-1" % (nwd, layout))
    _stayed_on_banded_kernel(st, events, nwd, WR.SYMS[layout])


@pytest.mark.parametrize("layout", WR.LAYOUTS)
@pytest.mark.parametrize("nwd", [3, 6])
def test_banded_paths_at_three_and_six_words(nwd, layout):
    """the word counts no other test runs on either layout, with start locations and alignments"""
    st, events = _run("banded:%d:%s:path:-1" % (nwd, layout))
    _stayed_on_banded_kernel(st, events, nwd, WR.SYMS[layout])
