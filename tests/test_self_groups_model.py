"""CPU: grouped self batches without a device -- the host layout and the lane predicate the kernel shares with it
(edlib_amd/csrc/self_groups_layout.hpp) run by tests/self_groups_host.cpp, a program of its own built with the address and
undefined-behaviour sanitizers and run as a child process; the numpy models of the counters and of the index mapping
against brute force; and the refusals Create makes before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edlib_amd
import self_groups_cases as SG
from test_self_model import self_word_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "self_groups_host.cpp")
HDR = os.path.join(ROOT, "edlib_amd", "csrc", "self_groups_layout.hpp")


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


def test_host_layout_runs_clean_under_sanitizers():
    """every wanted pair live exactly once, no other lane live inside the length window, every trip inside a run's range,
    wordSteps the sum over the live lanes: over 60 random sets and the planted cases; built with
    -fsanitize=address,undefined (without, where the toolchain links no sanitizer runtimes), as a child process.  The
    one-group cases' word_steps are held against the ungrouped formula of test_self_model.py."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "self_groups_host_san")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-static-libasan", "-static-libubsan"]
    if _stale(exe):
        probe = os.path.join(ROOT, "build", "sanitizer_probe")
        r = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
        if r.returncode != 0:
            flags = ["-O1", "-g", "-std=c++17"]
        r = subprocess.run(["g++"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "\n0 failures" in r.stdout, r.stdout[-4000:]
    seen = {m.group(1): {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", m.group(2))}
            for m in re.finditer(r"^case (\S+) (.*)$", r.stdout, re.M)}
    for name in ("sizes_k0", "sizes_k2", "big_group", "scattered", "singletons", "one_group_k0", "one_group_k3"):
        assert name in seen, name
    assert sum(name.startswith("random") for name in seen) == 60
    assert seen["singletons"]["items"] == 0 and seen["big_group"]["live"] > 500_000
    assert seen["small_groups"]["items"] > 65_535 and seen["small_groups"]["live"] == 600_000
    for name in ("one_group_k0", "one_group_k3"):
        c = seen[name]
        lengths = [20 + (i * 7) % 50 for i in range(c["n"])]
        assert c["word_steps"] == self_word_steps(lengths, c["k"]), name
        lo = np.minimum.outer(lengths, lengths)
        hi = np.maximum.outer(lengths, lengths)
        assert c["live"] == int(np.triu(hi - lo <= c["k"], 1).sum()), name


def _brute(lengths, groups, k):
    cells = steps = 0
    for i in range(len(lengths)):
        for j in range(i + 1, len(lengths)):
            if groups[i] != groups[j]:
                continue
            cells += lengths[i] * lengths[j]
            lo, hi = sorted((lengths[i], lengths[j]))
            if lo > 0 and hi <= 256 and hi - lo <= k:
                steps += (lo + 31) // 32 * hi
    return cells, steps


@pytest.mark.parametrize("n,labels", [(0, 1), (1, 1), (2, 1), (30, 1), (60, 4), (90, 40), (50, 500)])
def test_counter_models_match_brute_force(n, labels):
    rng = np.random.default_rng(n + labels)
    lengths = rng.choice([0, 1, 20, 31, 32, 33, 40, 64, 65, 256, 257, 300], size=n).tolist()
    groups = (rng.integers(-labels, labels, size=n) * 7919).tolist()
    for k in (0, 1, 8, 40):
        cells, steps = _brute(lengths, groups, k)
        assert SG.grouped_cells(lengths, groups) == cells
        assert SG.grouped_word_steps(lengths, groups, k) == steps
    first, second = SG.same_group_pairs(groups)
    want = [(i, j) for i in range(n) for j in range(i + 1, n) if groups[i] == groups[j]]
    assert list(zip(first.tolist(), second.tolist())) == want


def test_grouped_hits_model_maps_indices():
    """the mapping by hand: group 9 is the sequences 0, 2, 5, group -4 the sequences 1, 4, group 6 sequence 3 alone"""
    groups = [9, -4, 9, 6, -4, 9]
    per = {9: {"rowOffsets": [0, 2, 3, 3], "partner": [1, 2, 2], "editDistance": [1, 0, 2]},        # (0,2) (0,5) (2,5)
           -4: {"rowOffsets": [0, 1, 1], "partner": [1], "editDistance": [3]},                      # (1,4)
           6: {"rowOffsets": [0, 0], "partner": [], "editDistance": []}}
    got = edlib_amd.grouped_hits_model(groups, per)
    assert got["rowOffsets"].tolist() == [0, 2, 3, 4, 4, 4, 4]
    assert got["partner"].tolist() == [2, 5, 4, 5] and got["editDistance"].tolist() == [1, 0, 3, 2]
    assert got["partner"].dtype == np.int32 and got["rowOffsets"].dtype == np.int64
    empty = edlib_amd.grouped_hits_model([], {})
    assert empty["rowOffsets"].tolist() == [0] and len(empty["partner"]) == 0
    del per[-4]                                            # a group without an entry has no hits
    assert edlib_amd.grouped_hits_model(groups, per)["partner"].tolist() == [2, 5, 5]


def test_grouped_hits_model_matches_brute_force():
    rng = np.random.default_rng(2)
    for n, labels in ((40, 3), (80, 30)):
        groups = rng.integers(-labels, labels, size=n)
        d = rng.integers(-1, 3, size=(n, n))
        per = {}
        for lab, part in SG.members_of(groups).items():
            a, b = np.triu_indices(len(part), 1)
            per[lab] = SG.csr_of_pairs(len(part), a, b, d[part[a], part[b]])
        got = edlib_amd.grouped_hits_model(groups, per)
        first, second = SG.same_group_pairs(groups)
        want = SG.csr_of_pairs(n, first, second, d[first, second])
        for f in want:
            assert np.array_equal(got[f], want[f]), f


def test_planted_inputs_are_what_they_say():
    seqs, groups, planted = SG.planted_set()
    size = {lab: len(part) for lab, part in SG.members_of(groups).items()}
    assert sorted(size.values()) == list(SG.SIZES) and len(seqs) == sum(SG.SIZES)
    assert all(20 <= len(s) <= 43 for s in seqs)
    assert len({int(groups[i]) for i in planted["across"]}) == len(planted["across"]) == 5
    assert len({seqs[i] for i in planted["across"]}) == 1
    assert len({int(groups[i]) for i in planted["inside"]}) == 1 and len({seqs[i] for i in planted["inside"]}) == 1
    part = SG.members_of(groups)[SG.LABELS[8]]
    assert np.any(np.diff(part) > 1)                       # labels interleave: the group is not contiguous


def _create(groups=(1, 1), mode="NW", task="distance", k=1, null_groups=False):
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config(mode, task, k, None)
    s = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    o = np.array((0, 4, 8), dtype=np.int64)
    g = np.array(groups, dtype=np.int32)
    h = L.edlibAmdBatchCreateSelfHitsGrouped(s.ctypes.data, o.ctypes.data, 2, None if null_groups else g.ctypes.data, cfg, 0)
    err = edlib_amd.last_error()
    if h:
        L.edlibAmdBatchDestroy(h)
    return h, err


def test_symbol_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "edlib_amd.h")) as f:
        assert "edlibAmdBatchCreateSelfHitsGrouped(" in f.read()
    L = edlib_amd.lib()
    assert L.edlibAmdBatchCreateSelfHitsGrouped.restype is C.c_void_p


def test_refusals_before_the_device():
    h, err = _create(null_groups=True)
    assert not h and "groups is NULL" in err and "edlibAmdBatchCreateSelfHits" in err
    for k in (-1, -5):
        h, err = _create(k=k)
        assert not h and "config.k >= 0" in err and "no dense grouped form" in err
    for mode in ("HW", "SHW"):
        h, err = _create(mode=mode)
        assert not h and "EDLIB_MODE_NW" in err and mode in err and "cross batch" in err
    for task in ("locations", "path"):
        h, err = _create(task=task)
        assert not h and "EDLIB_TASK_DISTANCE" in err and "pair batch" in err
    L = edlib_amd.lib()
    cfg, _ = edlib_amd._make_config("NW", "distance", 1, None)
    g = np.zeros(3, dtype=np.int32)
    assert not L.edlibAmdBatchCreateSelfHitsGrouped(None, None, 3, g.ctypes.data, cfg, 0)
    assert "bad batch shape" in edlib_amd.last_error()
    o = np.array((0, 6, 4), dtype=np.int64)
    s = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    assert not L.edlibAmdBatchCreateSelfHitsGrouped(s.ctypes.data, o.ctypes.data, 2, g.ctypes.data, cfg, 0)
    assert "bad sequence offsets" in edlib_amd.last_error()


def test_python_refusals_name_the_remedy():
    seqs = [b"ACGT", b"ACGA"]
    with pytest.raises(ValueError, match="hits=True"):
        edlib_amd.SelfBatch(seqs, k=1, groups=[0, 0])
    with pytest.raises(ValueError, match="k >= 0"):
        edlib_amd.SelfBatch(seqs, hits=True, groups=[0, 0])
    with pytest.raises(ValueError, match="one-strand"):
        edlib_amd.SelfBatch(seqs, k=1, hits=True, strands="both", groups=[0, 0])
    with pytest.raises(ValueError, match="one label per sequence"):
        edlib_amd.SelfBatch(seqs, k=1, hits=True, groups=[0, 0, 0])
    with pytest.raises(ValueError, match="one label per sequence"):
        edlib_amd.SelfBatch(seqs, k=1, hits=True, groups=[0.5, 1.0])
    with pytest.raises(ValueError, match="return_inverse"):
        edlib_amd.SelfBatch(seqs, k=1, hits=True, groups=[0, 2**40])
    with pytest.raises(ValueError, match="k >= 0"):
        edlib_amd.knn(seqs, 2, groups=[0, 0])
    with pytest.raises(ValueError, match="k >= 0"):
        edlib_amd.cluster_within(seqs, -1, groups=[0, 0])
