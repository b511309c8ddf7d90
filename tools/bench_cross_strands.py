#!/usr/bin/env python3
"""What both strands cost in a cross batch: the demultiplexing shape -- 96 x 24 bp barcodes against N x 150 bp
reads, HW, at k = 3 and k = -1, every second read carrying its barcode reverse-complemented -- as
  (a) a both-strand batch of the 96 barcodes: run, then the BEST view and the strands of the best hits,
  (b) the way without it: a plain cross batch over the 192 host-made queries (barcode, reverse complement, ...), run, then
      the MATRIX view and the fold of the two strands in numpy (cross_strands_model),
  (c) the plain batch of the 96 barcodes on one strand, the yardstick.
The legs alternate in one process; medians of --runs resident runs after one warm-up each.  Checked without a clock: (a)'s
word_steps equal (b)'s and are twice (c)'s, and (a)'s combined cells and strand bytes equal the fold of (b)'s matrix on a
sample of cells.  One timing condition: the median scan_ms of (a) exceeds that of (b) -- the existing kernel over the same
192 slots -- by no more than the spread (max - min) (b) shows.  The exit status is 0 only if all of them hold.  One JSON
line, to stdout and to --out (default profiles/bench_cross_strands.json; with fewer legs than abc, the same name with the
legs appended, so that a partial run never replaces the full line).

Leg (b) on another build of the library: `EDLIB_AMD_LIB=/path/to/libedlib.so python tools/bench_cross_strands.py --legs b`,
started from this tree.  Leg (b) asks the library for nothing an older build lacks (the fold is numpy); legs (a) need this
build.  --baseline FILE puts such a line into the full record as "b_other_build" and holds (a)'s scan against it as well.

    python tools/bench_cross_strands.py [--reads 1000000] [--runs 5] [--legs abc] [--baseline FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import edlib_amd  # noqa: E402

FIELDS = ("editDistance", "numLocations", "endLocation")
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def inputs(rng, nreads, nbc=96, bclen=24, rlen=150):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = rng.choice(acgt, size=(nbc, bclen)).astype(np.uint8)
    reads = rng.choice(acgt, size=(nreads, rlen)).astype(np.uint8)
    which = rng.integers(0, nbc, size=nreads)
    planted = barcodes[which]
    planted[1::2] = COMP[planted[1::2, ::-1]]                      # every second read: the barcode on the other strand
    reads[:, 10:10 + bclen] = planted
    doubled = np.empty((2 * nbc, bclen), dtype=np.uint8)
    doubled[0::2] = barcodes
    doubled[1::2] = COMP[barcodes[:, ::-1]]
    return barcodes, doubled, reads, which


def fold(mat):
    fwd = {f: mat[f][:, 0::2] for f in FIELDS}
    rev = {f: mat[f][:, 1::2] for f in FIELDS}
    return edlib_amd.cross_strands_model(fwd, rev)


def one_k(barcodes, doubled, reads, which, k, runs, legs, sample, rng):
    make = {"a": lambda: edlib_amd.CrossBatch(barcodes, reads, mode="HW", k=k, strands="both"),
            "b": lambda: edlib_amd.CrossBatch(doubled, reads, mode="HW", k=k),
            "c": lambda: edlib_amd.CrossBatch(barcodes, reads, mode="HW", k=k)}
    batches = {x: make[x]() for x in legs}
    scan = {x: [] for x in legs}
    run = {x: [] for x in legs}
    view = {x: [] for x in legs}
    steps, kept = {}, {}
    try:
        for x in legs:
            batches[x].run()                                        # warm-up
        for _ in range(runs):
            for x in legs:
                b = batches[x]
                t0 = time.perf_counter()
                st = b.run()
                t1 = time.perf_counter()
                if x == "a":
                    kept["a_best"] = {f: v.copy() for f, v in b.best(copy=False).items()}
                    kept["a_best"].update(b.strands(cells=False))
                elif x == "b":
                    cells, strand = fold(b.matrix(copy=False))
                    kept["b_fold"] = (cells, strand)
                else:
                    b.best(copy=False)
                t2 = time.perf_counter()
                scan[x].append(st["scan_ms"]); run[x].append((t1 - t0) * 1e3); view[x].append((t2 - t1) * 1e3)
                steps[x] = st["word_steps"]
        out = {"k": k}
        for x in legs:
            out[x] = {"scan_ms": round(float(np.median(scan[x])), 3), "scan_ms_min": round(min(scan[x]), 3),
                      "scan_ms_max": round(max(scan[x]), 3), "run_ms": round(float(np.median(run[x])), 3),
                      "view_ms": round(float(np.median(view[x])), 3),
                      "end_to_end_ms": round(float(np.median(np.add(run[x], view[x]))), 3), "word_steps": steps[x]}
        ok = True
        if "a" in legs and "b" in legs:
            m = batches["a"].matrix(copy=False)
            s = batches["a"].strands(copy=False)["cellStrand"]
            cells, strand = kept["b_fold"]
            nt, nq = s.shape
            idx = rng.choice(nt * nq, size=min(sample, nt * nq), replace=False)
            t_, q_ = idx // nq, idx % nq
            bad = sum(int(np.sum(m[f][t_, q_] != cells[f][t_, q_])) for f in FIELDS) + int(np.sum(s[t_, q_] != strand[t_, q_]))
            spread = max(scan["b"]) - min(scan["b"])
            over = float(np.median(scan["a"]) - np.median(scan["b"]))
            # the calls: a read's barcode is found on the strand it was planted on (where the best is unique)
            best = kept["a_best"]
            unique = best["bestQueryDistance"] != best["secondQueryDistance"]
            called = int(np.sum((best["bestQuery"] == which) & unique))
            strand_ok = int(np.sum(((best["bestQueryStrand"] & 1) == (np.arange(len(which)) % 2))
                                   & (best["bestQuery"] == which) & unique))
            out["checks"] = {"word_steps_a_equal_b": steps["a"] == steps["b"], "sample_cells": int(len(idx)),
                             "sample_mismatches_a_vs_fold_of_b": bad, "scan_a_minus_b_ms": round(over, 3),
                             "scan_b_spread_ms": round(spread, 3), "scan_a_within_b_spread": over <= spread,
                             "reads_called_uniquely": called, "of_them_on_the_planted_strand": strand_ok}
            ok = ok and steps["a"] == steps["b"] and bad == 0 and over <= spread
        if "a" in legs and "c" in legs:
            out.setdefault("checks", {})["word_steps_a_twice_c"] = steps["a"] == 2 * steps["c"]
            ok = ok and steps["a"] == 2 * steps["c"]
        return out, ok
    finally:
        for b in batches.values():
            b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--sample", type=int, default=20_000)
    ap.add_argument("--baseline", help="the line of a --legs b run on another build of the library")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    barcodes, doubled, reads, which = inputs(rng, a.reads)
    legs = [x for x in "abc" if x in a.legs]
    if not a.out:
        name = "bench_cross_strands%s.json" % ("" if legs == list("abc") else "_" + "".join(legs))
        a.out = os.path.join(ROOT, "profiles", name)
    other = None
    if a.baseline:
        with open(a.baseline) as f:
            other = json.loads(f.readline())
        if other["shape"] != [len(barcodes), len(reads)] or other["runs"] != a.runs:
            sys.exit("--baseline: %s was measured on another shape or number of runs" % a.baseline)
    line = {"tool": "bench_cross_strands", "shape": [len(barcodes), len(reads)], "mode": "HW", "runs": a.runs,
            "legs": "".join(legs), "library": edlib_amd.LIB_PATH if os.environ.get("EDLIB_AMD_LIB") else "in-tree"}
    ok = True
    for k in (3, -1):
        line["k=%d" % k], good = one_k(barcodes, doubled, reads, which, k, a.runs, legs, a.sample, rng)
        ok = ok and good
        if other and "a" in legs:
            res, b = line["k=%d" % k], other["k=%d" % k]["b"]
            res["b_other_build"] = b
            over, spread = res["a"]["scan_ms"] - b["scan_ms"], b["scan_ms_max"] - b["scan_ms_min"]
            res.setdefault("checks", {}).update({"scan_a_minus_b_other_build_ms": round(over, 3),
                                                 "scan_b_other_build_spread_ms": round(spread, 3),
                                                 "scan_a_within_b_other_build_spread": over <= spread,
                                                 "word_steps_a_equal_b_other_build": res["a"]["word_steps"] == b["word_steps"]})
            ok = ok and over <= spread and res["a"]["word_steps"] == b["word_steps"]
    if other:
        line["other_build"] = other["library"]
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
