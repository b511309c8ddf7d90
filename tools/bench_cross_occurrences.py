"""Occurrence cross batches beside hit-list cross batches on one device: the demultiplexing shape (96 x 24 bp barcodes
against 1M x 150 bp reads, HW, k = 3) as CrossBatch(occurrences=True) and as CrossBatch(hits=True), both resident in one
process and run alternately; medians of `--runs` (5) of run_ms and scan_ms per leg, word_steps, the view time and the
hit counts, and the ratio of the two scan_ms medians -- the hit-list scan does the same column work, so it is the number
the occurrence scan is held against (DESIGN.md §4h "Occurrence batches").  Writes one JSON line to
profiles/bench_cross_occurrences.json and prints it.

    python tools/bench_cross_occurrences.py [--reads 1000000] [--runs 5] [--k 3] [--out profiles/bench_cross_occurrences.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import edlib_amd  # noqa: E402
from bench_cross import demux_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_cross_occurrences.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    bc, reads = demux_inputs(rng, a.reads)
    legs = {"occurrences": edlib_amd.CrossBatch(bc, reads, mode="HW", k=a.k, occurrences=True),
            "hits": edlib_amd.CrossBatch(bc, reads, mode="HW", k=a.k, hits=True)}
    res = {"metric": "bench_cross_occurrences", "shape": [len(bc), len(reads)], "k": a.k, "runs": a.runs}
    try:
        first = {n: b.run() for n, b in legs.items()}          # warm-up (a first run past the list's capacity grows it)
        ms = {n: [] for n in legs}
        scan = {n: [] for n in legs}
        last = {}
        for _ in range(a.runs):                                 # alternating: both legs see the same minutes of the box
            for n, b in legs.items():
                t = time.perf_counter()
                last[n] = b.run()
                ms[n].append((time.perf_counter() - t) * 1e3)
                scan[n].append(last[n]["scan_ms"])
        for n, b in legs.items():
            t = time.perf_counter()
            v = b.occurrences(copy=False) if n == "occurrences" else b.hits(copy=False)
            view_ms = (time.perf_counter() - t) * 1e3
            res[n] = {"run_ms": float(np.median(ms[n])), "scan_ms": float(np.median(scan[n])),
                      "scan_ms_all": [float(x) for x in scan[n]], "first_run_ms": first[n]["run_ms"],
                      "first_scan_launches": first[n]["scan_launches"], "view_ms": view_ms,
                      "numHits": int(len(v["query"])), "word_steps": last[n]["word_steps"], "cells": last[n]["cells"],
                      "scan_launches": last[n]["scan_launches"], "path": last[n]["path"]}
            if n == "occurrences":
                res[n]["cells_with_an_occurrence"] = int(len(np.unique(
                    np.repeat(np.arange(len(reads), dtype=np.int64), np.diff(v["targetOffsets"])) * len(bc) + v["query"])))
        res["scan_ms_ratio"] = res["occurrences"]["scan_ms"] / max(res["hits"]["scan_ms"], 1e-9)
    finally:
        for b in legs.values():
            b.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
