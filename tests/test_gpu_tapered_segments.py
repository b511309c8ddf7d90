"""-m gpu: the tapered segments of the last level's main launch (edlib_amd/csrc/segment_plan.hpp, engine_reads.hip).
The batch of tests/tapered_cases.py -- 16,384 reads of 150 bases, 256 read blocks, against 2,000,003 columns -- runs twice in
a child process with EDLIB_AMD_DEBUG=1.  The library's own lines say that every read reached the last level on the plain
kernel and that the launch had the planner's segment count (from ~7.8 k columns down to 1,280).

The planted reads sit 40 substitutions from the target: above every ladder level the run took (asserted from the "ladder"
line; an unrelated read's best is 54 .. 66, so the ladder prices no level for this batch) and below what random sequence
reaches, so the planted locations are the best ones (the reference confirms it).  They end in the shortest tail segment; on the last column of one segment
and on the first of the next, among the long and among the short segments; at two places in different segments; at 20
places inside one short segment (past the 16 positions a segment keeps: scanned again by the exact pass) and at 10 + 10
places around a boundary (past the slot's 16 only: gathered from the level's records); and on the target's last column.
Every field of the planted reads and of 200 strided unrelated ones is compared with the reference, for both runs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tapered_cases as TC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned \(plain=(\d)\)")
_LADDER_LINE = re.compile(r"ladder nwords=(\d+) kFirst=(\d+) open=(\d+)/(\d+) levels:((?: \d+\([0-9.]+\))*) full")
_SCAN_LINE = re.compile(r"scanGroup nwords=(\d+) mode=2 nlanes=(\d+) S=(\d+) segLen=(\d+) warm=(\d+) .* rows=(\w+)")


def test_planted_reads_on_tapered_segments(tmp_path):
    b = TC.batch()
    tab = b["table"]
    start, cols = tab[:, 0], tab[:, 1]
    assert cols[0] > 7000 and cols[-2] == 1280 and len(tab) > 256               # a real taper
    out = str(tmp_path / "child.npz")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tapered_child.py"), out],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    # ---- the library's own lines: both runs took every read to the last level, plain kernel, on the planner's segments
    levels = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in _LEVEL_LINE.finditer(p.stderr)]
    assert levels == [(0x3fffffff, TC.N, 1)] * 2, levels
    for m in _LADDER_LINE.finditer(p.stderr):
        assert all(int(t) < TC.SUBS for t in re.findall(r" (\d+)\(", m.group(5))), m.group(0)
    main = [m for m in _SCAN_LINE.finditer(p.stderr) if int(m.group(2)) == TC.N and m.group(6) == "delay" and int(m.group(3)) > 1]
    assert len(main) == 2 and all(int(m.group(3)) == len(tab) for m in main), [m.group(0) for m in main]
    # ---- the reference for the planted reads and 200 strided others
    names = sorted(b["planted"])
    sel = [b["planted"][n] for n in names] + [i for i in range(11, TC.N, TC.N // 200) if i not in b["planted"].values()][:200]
    sel = np.array(sel, dtype=np.int32)
    qoff = np.arange(TC.N + 1, dtype=np.int64) * TC.M
    ref = O.pool_align(np.concatenate(b["reads"]), qoff, b["target"], np.array([0, TC.T], dtype=np.int64), True, "HW",
                       "distance", -1, select=sel)
    print("reference: %d reads in %.2f s on %d threads" % (len(sel), ref["wall_seconds"], ref["threads"]))
    rlo = ref["locOff"]

    def seg_of(col):
        return int(np.searchsorted(start, col, side="right")) - 1

    # ---- the planted reads are where the plan put them (the reference says so)
    for j, n in enumerate(names):
        want = b["ends"][n]
        got_ends = ref["ends"][rlo[j]:rlo[j + 1]].tolist()
        # (a neighbouring column may tie through an indel; every planted column is among the best ones)
        assert ref["editDistance"][j] <= TC.SUBS and set(want) <= set(got_ends), (n, ref["editDistance"][j], got_ends, want)
        assert len(got_ends) <= len(want) + 2, (n, got_ends, want)
    e = b["ends"]
    assert seg_of(e["tail"][0]) == len(tab) - 2
    for kind in ("long", "short"):
        last, first = e[kind + "_last"][0], e[kind + "_first"][0]
        assert first == last + 1 and seg_of(first) == seg_of(last) + 1 and first == start[seg_of(first)]
        assert cols[seg_of(last)] == (cols[0] if kind == "long" else 1280)
    assert cols[seg_of(e["two_long_short"][0])] == cols[0] and cols[seg_of(e["two_long_short"][1])] == 1280
    assert seg_of(e["two_short_short"][1]) == seg_of(e["two_short_short"][0]) + 1
    assert len({seg_of(c) for c in e["many_in_one"]}) == 1 and len(e["many_in_one"]) > 16 and cols[seg_of(e["many_in_one"][0])] == 1280
    across = [seg_of(c) for c in e["many_across"]]
    assert across.count(across[0]) == 10 and across.count(across[0] + 1) == 10
    assert e["target_end"] == [TC.T - 1] and TC.T % 16 != 0 and seg_of(TC.T - 1) == len(tab) - 1
    # ---- every field, both runs
    got = np.load(out)
    for run in ("1", "2"):
        glo = got["locOff" + run]
        for j, u in enumerate(sel.tolist()):
            for f in ("status", "editDistance", "numLocations", "alphabetLength"):
                assert got[f + run][u] == ref[f][j], (run, u, f, got[f + run][u], ref[f][j])
            assert np.array_equal(got["ends" + run][glo[u]:glo[u + 1]], ref["ends"][rlo[j]:rlo[j + 1]]), (run, u)
        st = json.loads(str(got["stats" + run]))
        assert st["overflow_units"] >= 2, st                                 # many_in_one and many_across, at the least
    for f in ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends"):
        assert np.array_equal(got[f + "1"], got[f + "2"]), f
