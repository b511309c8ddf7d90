"""Grouped self batches (SelfBatch(hits=True, groups=...)) beside what a caller did without them, on one device; medians
of resident runs, the legs alternating in one process.

Leg A, the de-duplication shape with its families known: 200,000 x 32 bp in 2,000 families of 100, NW, k = 2, groups =
family -- the grouped run + hits view beside the ungrouped SelfBatch(hits=True) run + hits view + a numpy filter to the
same-family pairs.  The two hit sets must be equal (asserted); `faster` says whether the grouped way is shorter than the
old way by more than the spread (max - min) of the old way's own repeats.
Leg B, many small groups: 2,000,000 x 12 bp in about 400,000 groups of geometric size (mean 5), k = 1 -- Create, run,
scan, hits view and components() each on its own, and beside them a SelfBatch per group over 2,000 sampled groups (the
per-group time is measured; the time for all groups is that times their number, an extrapolation and labelled so).  The
work items and the live-lane share come from the layout itself (tools/self_groups_layout.cpp, built here with g++).
Prints one JSON line and writes profiles/bench_self_groups.json.

    python tools/bench_self_groups.py [--families 2000] [--sequences 2000000] [--sample 2000] [--runs 5]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import edlib_amd  # noqa: E402
from bench_cross import families  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def layout_counters(groups, lengths, k):
    """items, trips and live-lane share of the layout Create makes for this set (sequences of 1..256 bases)"""
    exe = os.path.join(ROOT, "build", "self_groups_layout")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "self_groups_layout.cpp")], check=True)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        np.array([len(groups)], dtype=np.int32).tofile(f)
        np.asarray(groups, dtype=np.int32).tofile(f)
        np.asarray(lengths, dtype=np.int32).tofile(f)
        f.flush()
        return json.loads(subprocess.run([exe, f.name, str(k)], check=True, capture_output=True, text=True).stdout)


def leg_a(a, rng):
    seqs = families(rng, a.families, 100)
    n = len(seqs)
    fam = np.repeat(np.arange(a.families), 100)
    order = rng.permutation(n)                             # families are not contiguous in the input
    seqs, fam = seqs[order], fam[order]
    g = edlib_amd.SelfBatch(seqs, k=2, hits=True, groups=fam)
    u = edlib_amd.SelfBatch(seqs, k=2, hits=True)

    def grouped():
        st = g.run()
        return st, g.hits(copy=False)

    def old_way():
        st = u.run()
        h = u.hits(copy=False)
        row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
        keep = fam[row] == fam[h["partner"]]
        return st, (row[keep], h["partner"][keep], h["editDistance"][keep])

    grouped(), old_way()                                   # warm-up: the hit lists grow here
    ms = {"grouped": [], "old": []}
    scan = {"grouped": [], "old": []}
    for _ in range(a.runs):
        (st_g, h), t = timed(grouped)
        ms["grouped"].append(t)
        scan["grouped"].append(st_g["scan_ms"])
        (st_u, kept), t = timed(old_way)
        ms["old"].append(t)
        scan["old"].append(st_u["scan_ms"])
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    assert np.array_equal(row, kept[0]) and np.array_equal(h["partner"], kept[1]) and np.array_equal(h["editDistance"], kept[2]), \
        "the grouped hits differ from the filtered ungrouped hits"
    spread = max(ms["old"]) - min(ms["old"])
    leg = {"shape": [n, 32], "families": a.families, "k": 2, "hits_equal": True, "numHits": int(len(h["partner"])),
           "grouped": {"run_plus_view_ms": float(np.median(ms["grouped"])), "all_ms": ms["grouped"],
                       "scan_ms": float(np.median(scan["grouped"])), "word_steps": st_g["word_steps"], "cells": st_g["cells"]},
           "old_way": {"run_plus_view_plus_filter_ms": float(np.median(ms["old"])), "all_ms": ms["old"], "spread_ms": spread,
                       "scan_ms": float(np.median(scan["old"])), "word_steps": st_u["word_steps"], "cells": st_u["cells"]}}
    leg["word_steps_ratio"] = st_g["word_steps"] / max(st_u["word_steps"], 1)
    leg["scan_ratio"] = leg["grouped"]["scan_ms"] / max(leg["old_way"]["scan_ms"], 1e-9)
    leg["time_ratio"] = leg["grouped"]["run_plus_view_ms"] / max(leg["old_way"]["run_plus_view_plus_filter_ms"], 1e-9)
    leg["faster"] = bool(leg["old_way"]["run_plus_view_plus_filter_ms"] - leg["grouped"]["run_plus_view_ms"] > spread)
    leg["layout"] = layout_counters(fam, np.full(n, 32), 2)
    g.close()
    u.close()
    return leg


def leg_b(a, rng):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    size = rng.geometric(1 / 5, size=int(a.sequences / 5 * 1.1) + 10)
    size = size[:np.searchsorted(np.cumsum(size), a.sequences) + 1]
    founders = rng.choice(acgt, size=(len(size), 12)).astype(np.uint8)
    seqs = np.repeat(founders, size, axis=0)
    groups = np.repeat(np.arange(len(size)), size)
    n = len(seqs)
    hit = rng.random(n) < 0.5                              # half of them one substitution away from the founder
    seqs[hit, rng.integers(0, 12, size=int(hit.sum()))] = rng.choice(acgt, size=int(hit.sum()))
    order = rng.permutation(n)
    seqs, groups = seqs[order], groups[order]
    leg = {"shape": [n, 12], "groups": int(len(size)), "mean_group": float(size.mean()), "k": 1}
    b, leg["create_ms"] = timed(lambda: edlib_amd.SelfBatch(seqs, k=1, hits=True, groups=groups))
    leg["first_run_ms"] = b.run()["run_ms"]
    ms, scan = [], []
    for _ in range(a.runs):
        st, t = timed(b.run)
        ms.append(t)
        scan.append(st["scan_ms"])
    leg["run_ms"], leg["scan_ms"], leg["all_run_ms"] = float(np.median(ms)), float(np.median(scan)), ms
    h, leg["view_hits_ms"] = timed(lambda: b.hits(copy=False))
    comp, leg["components_ms"] = timed(lambda: b.components(copy=False))
    leg["numHits"], leg["numComponents"] = int(len(h["partner"])), int(comp["numComponents"])
    leg["word_steps"], leg["scan_launches"] = st["word_steps"], st["scan_launches"]
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    assert np.all(groups[row] == groups[h["partner"]]) and np.all(groups[comp["label"]] == groups)
    # a SelfBatch per group over sampled groups: Create, run, hits view, close
    by = np.argsort(groups, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(groups))])
    pick = rng.choice(len(size), size=min(a.sample, len(size)), replace=False)
    parts = [seqs[by[cut[p]:cut[p + 1]]] for p in pick]
    hits_loop = 0

    def loop():
        nonlocal hits_loop
        for part in parts:
            s = edlib_amd.SelfBatch(part, k=1, hits=True)
            s.run()
            hits_loop += len(s.hits()["partner"])
            s.close()
    _, loop_ms = timed(loop)
    want = sum(int(((groups[row] == p)).sum()) for p in pick[:50])
    got50 = 0
    for part in parts[:50]:
        s = edlib_amd.SelfBatch(part, k=1, hits=True)
        s.run()
        got50 += len(s.hits()["partner"])
        s.close()
    assert got50 == want, "per-group batches list other hits than the grouped batch"
    leg["per_group_loop"] = {"sampled_groups": int(len(pick)), "ms_per_group": loop_ms / max(len(pick), 1),
                             "all_groups_ms_extrapolated": loop_ms / max(len(pick), 1) * len(size),
                             "note": "all_groups_ms_extrapolated is ms_per_group times the number of groups, not a measurement"}
    leg["layout"] = layout_counters(groups, np.full(n, 12), 1)
    b.close()
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=2000, help="families of 100 in the 32 bp shape")
    ap.add_argument("--sequences", type=int, default=2_000_000, help="sequences of the many-small-groups shape")
    ap.add_argument("--sample", type=int, default=2000, help="groups of the per-group loop")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"metric": "bench_self_groups"}
    res["families_200k_32"] = leg_a(a, rng)
    res["small_groups_2m_12"] = leg_b(a, rng)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_self_groups.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
