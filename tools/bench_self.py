"""Self batches (one set against itself, every unordered pair once) beside the cross batch given the same pool twice, on
one device; medians of resident runs, the two legs alternating in one process.

Leg 1, the de-duplication shape: 200,000 x 32 bp in 2,000 families of 100, NW, k = 2 -- SelfBatch(hits=True) beside
CrossBatch(seqs, seqs, hits=True).  By the counters the self scan is (n - 1) / 2n of the cross scan; scan_ratio is the
measured scan_ms ratio (required: <= 0.60).
Leg 2, the distance-matrix shape: 2,000 x 150 bp amplicons, NW, dense -- the SELF_DISTANCES view beside the cross MATRIX
view (one int array of half the cells against three full ones).
Sampled distances of both legs are checked against the reference.  Prints one JSON line and writes
profiles/bench_self.json.

    python tools/bench_self.py [--families 2000] [--amplicons 2000] [--runs 5] [--check 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import edlib_amd  # noqa: E402
from bench_cross import amplicons, families  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def alternate(legs, runs):
    """legs: {name: batch}.  One warm-up run each (a hit list grows there), then `runs` rounds of one run per leg."""
    first = {name: b.run()["run_ms"] for name, b in legs.items()}
    ms = {name: [] for name in legs}
    scan = {name: [] for name in legs}
    st = {}
    for _ in range(runs):
        for name, b in legs.items():
            st[name], wall = timed(b.run)
            ms[name].append(wall)
            scan[name].append(st[name]["scan_ms"])
    return {name: {"run_ms": float(np.median(ms[name])), "scan_ms": float(np.median(scan[name])),
                   "first_run_ms": first[name], "cells": st[name]["cells"], "word_steps": st[name]["word_steps"],
                   "scan_launches": st[name]["scan_launches"], "path": st[name]["path"]} for name in legs}


def mismatches(seqs, i, j, got, k):
    from oracle import oracle as O

    def pack(s):
        off = np.zeros(len(s) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in s])
        return np.frombuffer(b"".join(s) + b"\0", dtype=np.uint8), off
    qp, qo = pack([bytes(seqs[int(a)]) for a in i])
    tp, to = pack([bytes(seqs[int(b)]) for b in j])
    r = O.pool_align(qp, qo, tp, to, False, "NW", "distance", k)
    return int(np.sum(np.asarray(r["editDistance"]) != got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=2000, help="families of 100 in the 32 bp shape")
    ap.add_argument("--amplicons", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=2000)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"metric": "bench_self"}

    # ---- leg 1: hits
    seqs = families(rng, a.families, 100)
    n = len(seqs)
    s = edlib_amd.SelfBatch(seqs, k=2, hits=True)
    c = edlib_amd.CrossBatch(seqs, seqs, mode="NW", k=2, hits=True)
    leg = alternate({"self": s, "cross": c}, a.runs)
    h, leg["self"]["view_hits_ms"] = timed(lambda: s.hits(copy=False))
    _, leg["self"]["view_nearest_ms"] = timed(lambda: s.nearest(copy=False))
    ch, leg["cross"]["view_hits_ms"] = timed(lambda: c.hits(copy=False))
    leg["self"]["numHits"] = int(len(h["partner"]))
    leg["cross"]["numHits"] = int(len(ch["query"]))
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    pick = rng.choice(len(row), size=min(a.check, len(row)), replace=False)
    leg["sample_mismatches"] = mismatches(seqs, row[pick], h["partner"][pick], h["editDistance"][pick], 2)
    leg["hits_agree"] = bool(2 * leg["self"]["numHits"] + n == leg["cross"]["numHits"])
    leg["shape"] = [n, 32]
    leg["k"] = 2
    leg["scan_ratio"] = leg["self"]["scan_ms"] / max(leg["cross"]["scan_ms"], 1e-9)
    leg["run_ratio"] = leg["self"]["run_ms"] / max(leg["cross"]["run_ms"], 1e-9)
    leg["word_steps_ratio"] = leg["self"]["word_steps"] / max(leg["cross"]["word_steps"], 1)
    leg["scan_ratio_required"] = 0.60
    res["hits_200k_32"] = leg
    s.close()
    c.close()
    del h, ch, row

    # ---- leg 2: dense
    amp = amplicons(rng, a.amplicons)
    m = len(amp)
    s = edlib_amd.SelfBatch(amp)
    c = edlib_amd.CrossBatch(amp, amp, mode="NW")
    leg = alternate({"self": s, "cross": c}, a.runs)
    cond, leg["self"]["view_distances_ms"] = timed(lambda: s.condensed(copy=False))
    _, leg["self"]["view_nearest_ms"] = timed(lambda: s.nearest(copy=False))
    mat, leg["cross"]["view_matrix_ms"] = timed(lambda: c.matrix(copy=False))
    leg["self"]["view_bytes"] = int(cond.nbytes)
    leg["cross"]["view_bytes"] = int(sum(v.nbytes for v in mat.values()))
    i, j = np.triu_indices(m, 1)
    leg["equals_cross"] = bool(np.array_equal(mat["editDistance"][j, i], cond))
    pick = rng.choice(len(i), size=min(a.check, len(i)), replace=False)
    leg["sample_mismatches"] = mismatches(amp, i[pick], j[pick], cond[pick], -1)
    leg["shape"] = [m, 150]
    leg["view_bytes_ratio"] = leg["self"]["view_bytes"] / max(leg["cross"]["view_bytes"], 1)
    leg["view_ms_ratio"] = leg["self"]["view_distances_ms"] / max(leg["cross"]["view_matrix_ms"], 1e-9)
    leg["scan_ratio"] = leg["self"]["scan_ms"] / max(leg["cross"]["scan_ms"], 1e-9)
    res["dense_2000_150"] = leg
    s.close()
    c.close()

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_self.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
