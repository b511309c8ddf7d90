"""-m gpu: the exact pass of HW read groups without its rescans, and a seeded step without its probe (engine_reads.hip:
runGroupScans / runGroupExact).  A slot with more than 16 end locations gets its complete list GATHERED from the
segment records of the scan that answered it when every segment holding the best score kept all of its hits; only a slot
with a segment past its cap (8 in pass 1, 16 in the last level) is scanned again.

Every batch of tests/overflow_cases.py runs in a child process with EDLIB_AMD_DEBUG=1: every field against the reference,
the library's `exact pass nwords=N: a gathered, b rescanned` line against numbers computed on the CPU from the REFERENCE's
end locations and the segmentation the engine printed (`scanGroup ... S= segLen= cap=`), and Stats.scan_launches against
the launches a step needs.

Left out, as a fixed list: groups of more than one level after pass 1 that also overflow (the levels below the last keep
8 positions per segment and are rescanned: nothing new), SHW / NW (one segment, no gather), long reads (own merge)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import overflow_cases as OC
import seed_model as SM
from seed_model import seed_threshold
from test_gpu_seed_filter import _FIELDS, _nslots, _reference

pytestmark = pytest.mark.gpu

_SCAN_LINE = re.compile(r"scanGroup nwords=(\d+) mode=2 nlanes=(\d+) S=(\d+) segLen=(\d+) warm=\d+ cap=(\d+) kcap=(\d+) slotmap=(\S+) posOff=(\S+)")
_SEED_LINE = re.compile(r"seed pass nwords=(\d+) k=(-?\d+): (\d+) of (\d+) slots handed back")
_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned \(plain=(\d)\)")
_LADDER_LINE = re.compile(r"ladder nwords=(\d+) kFirst=(\d+) open=(\d+)/(\d+) levels:((?: \d+\([0-9.]+\))*) full")
_EXACT_LINE = re.compile(r"exact pass nwords=(\d+): (\d+) gathered, (\d+) rescanned")
_KNOCAP = 0x3fffffff


def _child(name, tmp_path):
    """runs the batch in a fresh process; returns the batch, the reference, the stats and the library's lines"""
    out = str(tmp_path / "child.npz")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "overflow_child.py"), name, out],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    log = {"scans": [], "seed": None, "levels": [], "ladder": None, "exact": None}
    for line in p.stderr.splitlines():
        m = _SCAN_LINE.search(line)
        if m:
            log["scans"].append({"nlanes": int(m.group(2)), "S": int(m.group(3)), "segLen": int(m.group(4)), "cap": int(m.group(5)),
                                 "kcap": int(m.group(6)), "map": m.group(7) != "(nil)", "exact": m.group(8) != "(nil)"})
        m = _SEED_LINE.search(line)
        if m:
            assert log["seed"] is None
            log["seed"] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
        m = _LEVEL_LINE.search(line)
        if m:
            log["levels"].append((int(m.group(1)), int(m.group(2)), int(m.group(3))))
        m = _LADDER_LINE.search(line)
        if m:
            log["ladder"] = (int(m.group(2)), int(m.group(3)), int(m.group(4)), [int(x) for x in re.findall(r" (\d+)\(", m.group(5))])
        m = _EXACT_LINE.search(line)
        if m:
            assert log["exact"] is None
            log["exact"] = (int(m.group(2)), int(m.group(3)))
    b = OC.batch(name)
    assert {(len(r) + 31) // 32 for r in b["reads"]} == {5}                    # one group of five words
    got = np.load(out)
    ref = _reference(b)
    for f in _FIELDS:
        assert np.array_equal(got[f], ref[f]), (name, f)
    if b["task"] != "distance":
        assert np.array_equal(got["starts"], ref["starts"]), name
    st = json.loads(str(got["stats"]))
    print(name, {k: v for k, v in log.items() if k != "scans"}, log["scans"][:8], st)
    return b, ref, st, log


def _last_level(log, leftovers):
    """the main launch of the last level: dense lanes (no slot map), 16 positions per segment, no threshold cap"""
    hit = [s for s in log["scans"] if s["nlanes"] == leftovers and s["cap"] == OC.CAP_LAST and not s["map"] and s["S"] > 1]
    assert len(hit) == 1 and hit[0]["kcap"] == _KNOCAP, log["scans"]
    return hit[0]


def _planted_claims(b, ref, k_first):
    """the planted reads are what the case says, by the reference alone: blocks with 17 / 40 / 64 end locations at
    distance 0, 3 and 10 .. 12 (every copy), tandem reads with more than 16 end locations five columns apart"""
    lo = ref["locOff"]
    seen = set()
    for u, c in enumerate(b["claims"]):
        if c is None:
            continue
        d, ends = int(ref["editDistance"][u]), ref["ends"][lo[u]:lo[u + 1]]
        assert d in (0, 3) or k_first < 10 <= d <= 12, (u, c, d)
        if c:
            # (every copy, and at most two neighbouring columns that tie after substitutions)
            assert c <= len(ends) <= 3 * c and len(np.unique((ends - ends[0] + 4) // 1_600)) == c, (u, c, len(ends))
            assert np.all((ends - ends[0] + 4) % 1_600 < 8), (u, c)
        else:
            assert len(ends) > 2 * OC.CAP_FINAL and np.sum(np.diff(ends) == 5) >= len(ends) - 2, (u, len(ends))
        seen.add((c, d <= k_first))
    assert seen == {(c, p) for c in (0, 17, 40, 64) for p in (False, True)}


@pytest.mark.parametrize("task", ["distance", "locations", "path"])
def test_seeded_group(task, tmp_path):
    """the seed filter answers pass 1 (its overflows are rescanned: it keeps no records); the blocks with 12 substitutions
    are leftovers of the last level and are gathered, the tandem reads are rescanned"""
    b, ref, st, log = _child("planted:" + task, tmp_path)
    T, n = len(b["target"]), len(b["reads"])
    assert 1_024 <= _nslots(n) < 16_384 and _nslots(n) * T >= 1 << 30
    K = log["seed"][0]
    assert K == seed_threshold(min(len(r) for r in b["reads"]), T) and 3 < K < 12
    _planted_claims(b, ref, K)
    leftovers = int(np.sum(ref["editDistance"] > K))
    assert log["levels"] == [(_KNOCAP, leftovers, log["levels"][0][2])] and log["ladder"] is None
    seg = _last_level(log, leftovers)
    want = OC.expected_exact_pass(ref, range(n), K, True, None, seg["segLen"])
    assert want[0] >= 6 and want[1] >= 8, want                     # both ways are in the batch
    assert log["exact"] == want, (log["exact"], want)
    assert st["overflow_units"] == sum(want) == int(np.sum(ref["numLocations"] > OC.CAP_FINAL)), st


@pytest.mark.parametrize("task", ["distance", "locations", "path"])
def test_group_without_the_filter(task, tmp_path):
    """a five-symbol target: banded pass 1 at threshold 8 with 8 positions per segment.  Blocks within it are gathered from
    the group's own records, blocks above it from the last level's, tandem reads are rescanned from both"""
    b, ref, st, log = _child("planted5:" + task, tmp_path)
    n = len(b["reads"])
    assert len(set(b["target"].tolist())) == 5 and log["seed"] is None and _nslots(n) < 16_384
    k_first = 8
    _planted_claims(b, ref, k_first)
    pass1 = log["scans"][0]
    assert pass1["nlanes"] == _nslots(n) and pass1["cap"] == OC.CAP_PASS1 and pass1["kcap"] == k_first and not pass1["map"]
    leftovers = int(np.sum(ref["editDistance"] > k_first))
    assert [lv[:2] for lv in log["levels"]] == [(_KNOCAP, leftovers)]
    seg = _last_level(log, leftovers)
    want = OC.expected_exact_pass(ref, range(n), k_first, False, pass1["segLen"], seg["segLen"])
    assert want[0] >= 12 and want[1] >= 4, want
    assert log["exact"] == want, (log["exact"], want)
    assert st["overflow_units"] == sum(want), st


def _launch_case(name, tmp_path):
    b, ref, st, log = _child(name, tmp_path)
    T, n = len(b["target"]), len(b["reads"])
    assert _nslots(n) >= 16_384 and _nslots(n) * T >= 1 << 30
    K, back, slots = log["seed"]
    assert K == seed_threshold(min(len(r) for r in b["reads"]), T) and back == 0 and slots == _nslots(n)
    return b, ref, st, log, K, int(np.sum(ref["editDistance"] > K))


def test_five_launches(tmp_path):
    """fewer than a tenth open, >= 4096 leftovers, no read with a crowded segment: index, seed pass, census, threshold scan,
    leftovers -- no probe, no exact scans"""
    b, ref, st, log, K, open_ = _launch_case("launches:few", tmp_path)
    assert 4_096 <= open_ and open_ * 10 <= len(b["reads"])
    seg = _last_level(log, open_)
    want = OC.expected_exact_pass(ref, range(len(b["reads"])), K, True, None, seg["segLen"])
    assert want[1] == 0, want
    assert log["ladder"] is None and log["levels"] == [(_KNOCAP, open_, 1)]
    assert (log["exact"] or (0, 0)) == want
    assert st["scan_launches"] == 5, st


def test_seven_launches_with_a_crowded_segment(tmp_path):
    """the same with three reads whose 40 end locations crowd one segment: the counting and the writing scan on top"""
    b, ref, st, log, K, open_ = _launch_case("launches:crowded", tmp_path)
    assert 4_096 <= open_ and open_ * 10 <= len(b["reads"])
    assert sum(p["back"] for p in SM.predict_batch(b["reads"][-3:], b["target"], K)) == 0       # (the filter keeps them)
    lo = ref["locOff"]
    for u in range(len(b["reads"]) - 3, len(b["reads"])):
        assert ref["editDistance"][u] == 12 and lo[u + 1] - lo[u] == 40
    seg = _last_level(log, open_)
    want = OC.expected_exact_pass(ref, range(len(b["reads"])), K, True, None, seg["segLen"])
    assert want[1] >= 3, want
    assert log["exact"] == want
    assert st["scan_launches"] == 7, st
    assert sum(1 for s in log["scans"] if s["exact"]) == 1 and log["scans"][-1]["nlanes"] == want[1]


def test_more_than_a_tenth_open_adds_the_ladder_sample(tmp_path):
    """13 % unrelated: one scan of at most 2048 open slots prices the ladder, then its levels"""
    b, ref, st, log, K, open_ = _launch_case("launches:open", tmp_path)
    assert open_ * 10 > len(b["reads"])
    kfirst, a, real, levels = log["ladder"]
    assert kfirst == K and (a, real) == (open_, len(b["reads"])) and all(t > K for t in levels)
    sample = log["scans"][0]
    assert sample["map"] and sample["nlanes"] == min(2_048, open_) and sample["kcap"] == min(64, 32 * 5 - 1)
    last = int(np.sum(ref["editDistance"] > (max(levels) if levels else K)))
    assert last >= 4_096 and len(log["levels"]) == len(levels) + 1 and log["levels"][-1][:2] == (_KNOCAP, last)
    seg_levels = {}
    for t in levels:
        hit = [s for s in log["scans"] if s["kcap"] == t and not s["map"] and s["cap"] == OC.CAP_PASS1]
        assert len(hit) == 1, (t, log["scans"])
        seg_levels[t] = hit[0]["segLen"]
    want = OC.expected_exact_pass(ref, range(len(b["reads"])), K, True, None, _last_level(log, last)["segLen"], seg_levels)
    assert (log["exact"] or (0, 0)) == want
    assert st["scan_launches"] == 5 + 1 + len(levels) + (2 if want[1] else 0), st
