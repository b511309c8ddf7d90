"""Components of a self batch labelled on the device (SelfBatch.components()) beside what a caller did before: fetch the
hit list and run connected components on the host.  The shape is the self batch's de-duplication shape -- 200,000 x 32 bp
in 2,000 families of 100, NW, k = 2, hit list -- on one strand and on both.

Per round, after a Run of the resident batch, in alternating order:
  (a) components() for the labels only, and with the members;
  (b) hits(copy=False) -- the first view of the Run, so the list crosses the link -- and then connected components over it
      on the host (scipy.sparse.csgraph where it imports, else self_components_model()).
Medians of `--runs` rounds; the labels of (a) and (b) are asserted equal.  The bar: (a) below the hits() view alone, by more
than the spread of the rounds.  The three kernels' times (hook, flatten, sizes) come from one rocprofv3 --kernel-trace
--stats run of a child process of their own (`--trace-child`), beside the bytes the hook kernel reads.
Prints one JSON line and writes profiles/bench_self_components.json.

    python tools/bench_self_components.py [--families 2000] [--runs 5] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
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


def host_labels(n, h):
    """what a caller ran over pairs_within(): the smallest index of every sequence's component"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return edlib_amd.self_components_model(n, h["rowOffsets"], h["partner"], h["editDistance"], -1)["label"], "model"
    row = np.repeat(np.arange(n, dtype=np.int32), np.diff(h["rowOffsets"]))
    g = coo_matrix((np.ones(len(row), dtype=np.int8), (row, h["partner"])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    first = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32), "scipy"


def leg(seqs, strands, runs):
    n = len(seqs)
    b = edlib_amd.SelfBatch(seqs, k=2, hits=True, strands=strands)
    try:
        b.run()                                                      # (the list grows here)
        b.components(members=True)                                   # (the buffers are made here)
        ms = {f: [] for f in ("run", "labels", "members", "hits_view", "host_components")}
        how = ""
        for r in range(runs):
            _, t = timed(b.run)
            ms["run"].append(t)

            def device():
                c, t1 = timed(lambda: b.components(copy=False))
                label = c["label"].copy()
                cm, t2 = timed(lambda: b.components(members=True, copy=False))
                ms["labels"].append(t1)
                ms["members"].append(t2)
                return label, cm["numComponents"]

            def host():
                h, t1 = timed(lambda: b.hits(copy=False))
                (label, how), t2 = timed(lambda: host_labels(n, h))
                ms["hits_view"].append(t1)
                ms["host_components"].append(t2)
                return label, how, int(len(h["partner"]))
            if r % 2 == 0:
                (dl, nc), (hl, how, nh) = device(), host()
            else:
                (hl, how, nh), (dl, nc) = host(), device()
            assert np.array_equal(dl, hl), "device and host labels differ"
        med = {f + "_ms": float(np.median(v)) for f, v in ms.items()}
        spread = {f + "_ms": [float(min(v)), float(max(v))] for f, v in ms.items()}
        out = {"shape": [n, 32], "k": 2, "strands": strands, "numHits": nh, "numComponents": int(nc), "host": how,
               "median": med, "min_max": spread,
               "device_bytes_over_link": {"labels": (2 * n + 1) * 4, "members": (4 * n + 3) * 4},
               "hits_bytes_over_link": (n + 1) * 8 + 2 * nh * 4,
               # per hit the sorted key, the partner and the distance (parent[] beside them: n ints, re-read from L2)
               "hook_bytes_read": nh * (8 + 4 + 4)}
        margin = spread["hits_view_ms"][1] - spread["hits_view_ms"][0]
        out["bar"] = "components() for labels below the hits() view alone, by more than the view's min-max spread"
        out["bar_met"] = bool(med["labels_ms"] + margin < med["hits_view_ms"])
        out["today_ms"] = med["hits_view_ms"] + med["host_components_ms"]
        return out
    finally:
        b.close()


def trace_child(n_families):
    """what the traced child runs: one batch, one Run, five components() calls with members"""
    seqs = families(np.random.default_rng(1), n_families, 100)
    b = edlib_amd.SelfBatch(seqs, k=2, hits=True)
    try:
        b.run()
        for _ in range(5):
            b.components(members=True)
    finally:
        b.close()


def kernel_times(n_families):
    """average ns of the self_components kernels from rocprofv3's kernel stats of a child of its own"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"not_measured": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="self_components_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
                            sys.executable, os.path.abspath(__file__), "--trace-child", "--families", str(n_families)],
                           capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"not_measured": "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-300:])}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                m = re.search(r"self_components_(\w+?)_kernel", row.get("Name", ""))
                if m:
                    out[m.group(1)] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
        return out or {"not_measured": "no self_components kernel in the stats"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=2000, help="families of 100 in the 32 bp shape")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.families)
        return
    seqs = families(np.random.default_rng(1), a.families, 100)
    res = {"metric": "bench_self_components", "runs": a.runs}
    res["forward"] = leg(seqs, "forward", a.runs)
    res["both_strands"] = leg(seqs, "both", a.runs)
    res["kernels"] = {"not_measured": "--no-trace"} if a.no_trace else kernel_times(a.families)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_self_components.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
