"""The K nearest neighbours selected on the device (SelfBatch.neighbors(), CrossBatch.neighbors()) beside what a caller
did before: fetch the hits() / condensed() / matrix() view and select on the host.  Shapes:
  self_hits        200,000 x 32 bp in 2,000 families of 100, NW k = 2, hit list, K = 10 and K = 64, one strand and both
  self_dense       2,000 x 150 bp amplicons, NW, dense, K = 10
  cross_dense/hits 96 x 24 bp barcodes against 1M x 150 bp reads, HW k = 3, dense and hit list, K = 3

Per round, after a Run of the resident batch, in alternating order:
  (a) neighbors(K, copy=False): the launches and the one copy;
  (b) the view (copy=False, the first view of the Run, so the data crosses the link) and the selection on the host: the
      numpy model (neighbors_model: one lexsort) or np.argpartition per row, whichever was faster in a round of its own
      in front of the timed ones.
Medians of `--runs` rounds; the outputs of (a) and (b) are asserted equal.  The aim: (a) shorter than (b) as a whole by
more than the difference between the two halves of (b)'s own rounds.
run_ms of the same batches is measured in child processes of their own, this build twice and -- with --parent-lib, a
libedlib.so of the parent commit loaded through EDLIB_AMD_LIB -- the parent once between them: Run gains no work, so the
parent's figure must lie within the two legs' own difference.
The kernels' times (degree count, scan, scatter, select) come from one rocprofv3 --kernel-trace --stats run of a child
process of their own.  Prints one JSON line and writes profiles/bench_neighbors.json.

    python tools/bench_neighbors.py [--families 2000] [--amplicons 2000] [--reads 1000000] [--runs 5] [--parent-lib PATH]
                                    [--no-trace] [--out profiles/bench_neighbors.json]
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
from bench_cross import amplicons, demux_inputs, families  # noqa: E402

FIELDS = ("count", "neighbor", "distance")
BIG = np.int64(1) << 62


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


# ---- the selection on the host, two ways

def rows_from_keys(key, K):
    """key int64 [rows, width], BIG where there is no candidate: the K smallest of every row by np.argpartition, sorted"""
    rows, width = key.shape
    if width > K:
        part = np.argpartition(key, K - 1, axis=1)[:, :K]
        key = np.take_along_axis(key, part, axis=1)
    key = np.sort(key, axis=1)
    if key.shape[1] < K:
        key = np.concatenate([key, np.full((rows, K - key.shape[1]), BIG, dtype=np.int64)], axis=1)
    have = key < BIG
    return {"count": have.sum(axis=1).astype(np.int32),
            "neighbor": np.where(have, key & 0xffffffff, -1).astype(np.int32),
            "distance": np.where(have, key >> 32, -1).astype(np.int32)}


def select_matrix(ed, K, how):
    """ed int32 [rows, width] (-1: none)"""
    rows, width = ed.shape
    if how == "model":
        t, q = np.divmod(np.arange(rows * width), width)
        return edlib_amd.neighbors_model(rows, t, q, ed.reshape(-1), K, -1)
    key = np.where(ed >= 0, (ed.astype(np.int64) << 32) | np.arange(width, dtype=np.int64)[None, :], BIG)
    return rows_from_keys(key, K)


def select_condensed(n, cond, K, how):
    i, j = np.triu_indices(n, 1)
    if how == "model":
        return edlib_amd.neighbors_model(n, np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([cond, cond]), K, -1)
    sq = np.full((n, n), -1, dtype=np.int32)
    sq[i, j] = cond
    sq[j, i] = cond
    return select_matrix(sq, K, "argpartition")


def select_csr(rows, off, partner, ed, K, how, mirror):
    """a CSR list; mirror: every entry also under its partner (a self batch's i < j list)"""
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(off))
    p, d = partner.astype(np.int64), ed.astype(np.int64)
    if mirror:
        row, p, d = np.concatenate([row, p]), np.concatenate([p, row]), np.concatenate([d, d])
    if how == "model":
        return edlib_amd.neighbors_model(rows, row, p, d, K, -1)
    # np.argpartition per row: the rows made contiguous by one stable sort, then a loop over them
    if mirror:
        order = np.argsort(row, kind="stable")
        row, p, d = row[order], p[order], d[order]
    key = (d << 32) | p
    start = np.searchsorted(row, np.arange(rows + 1))
    out = np.full((rows, K), BIG, dtype=np.int64)
    for r in range(rows):
        k = key[start[r]:start[r + 1]]
        if len(k) > K:
            k = k[np.argpartition(k, K - 1)[:K]]
        out[r, :len(k)] = np.sort(k)
    return rows_from_keys(out, K)


# ---- a shape: the batch, its old way, the Ks

class Shape:
    def __init__(self, name, make, view, select, Ks, note):
        self.name, self.make, self.view, self.select, self.Ks, self.note = name, make, view, select, Ks, note


def shapes(a):
    rng = np.random.default_rng(1)
    seqs = families(rng, a.families, 100)
    n = len(seqs)
    amp = amplicons(np.random.default_rng(2), a.amplicons)
    na = len(amp)
    barcodes, reads = demux_inputs(np.random.default_rng(3), a.reads)
    nt = len(reads)
    out = []
    for strands in ("forward", "both"):
        out.append(Shape("self_hits_" + strands,
                         lambda s=strands: edlib_amd.SelfBatch(seqs, k=2, hits=True, strands=s),
                         lambda b: b.hits(copy=False),
                         lambda h, K, how: select_csr(n, h["rowOffsets"], h["partner"], h["editDistance"], K, how, True),
                         (10, 64), "%d x 32 bp in %d families of 100, NW k = 2, hit list, %s" % (n, a.families, strands)))
    out.append(Shape("self_dense", lambda: edlib_amd.SelfBatch(amp, k=-1), lambda b: b.condensed(copy=False),
                     lambda c, K, how: select_condensed(na, c, K, how), (10,),
                     "%d x 150 bp amplicons, NW, dense" % na))
    out.append(Shape("cross_dense", lambda: edlib_amd.CrossBatch(barcodes, reads, mode="HW", k=3),
                     lambda b: b.matrix(copy=False), lambda m, K, how: select_matrix(m["editDistance"], K, how), (3,),
                     "96 x 24 bp barcodes against %d x 150 bp reads, HW k = 3, dense" % nt))
    out.append(Shape("cross_hits", lambda: edlib_amd.CrossBatch(barcodes, reads, mode="HW", k=3, hits=True),
                     lambda b: b.hits(copy=False),
                     lambda h, K, how: select_csr(nt, h["targetOffsets"], h["query"], h["editDistance"], K, how, False), (3,),
                     "96 x 24 bp barcodes against %d x 150 bp reads, HW k = 3, hit list" % nt))
    return out


def leg(s, runs):
    b = s.make()
    try:
        b.run()                                                      # (a hit list grows here)
        for K in s.Ks:
            b.neighbors(K)                                           # (the buffers are made here)
        # which host selection is the faster: a round of its own
        v = s.view(b)
        how_ms = {how: timed(lambda: s.select(v, s.Ks[0], how))[1] for how in ("model", "argpartition")}
        how = min(how_ms, key=how_ms.get)
        ms = {"run": [], "view": []}
        for K in s.Ks:
            ms["neighbors_K%d" % K], ms["host_select_K%d" % K] = [], []
        for r in range(runs):
            st, t = timed(b.run)
            ms["run"].append(st["run_ms"])

            def device():
                got = {}
                for K in s.Ks:
                    g, t1 = timed(lambda: b.neighbors(K, copy=False))
                    ms["neighbors_K%d" % K].append(t1)
                    got[K] = {f: g[f].copy() for f in FIELDS}
                return got

            def host():
                v, t1 = timed(lambda: s.view(b))
                ms["view"].append(t1)
                got = {}
                for K in s.Ks:
                    got[K], t2 = timed(lambda: s.select(v, K, how))
                    ms["host_select_K%d" % K].append(t2)
                return got
            d, h = (device(), host()) if r % 2 == 0 else (host(), device())[::-1]
            for K in s.Ks:
                for f in FIELDS:
                    assert np.array_equal(d[K][f], h[K][f]), "device and host differ: %s K = %d %s" % (s.name, K, f)
        med = {f + "_ms": float(np.median(x)) for f, x in ms.items()}
        out = {"shape": s.note, "host_selection": how, "host_selection_round_ms": how_ms, "median": med,
               "min_max": {f + "_ms": [float(min(x)), float(max(x))] for f, x in ms.items()}, "K": {}}
        for K in s.Ks:
            old = np.array(ms["view"]) + np.array(ms["host_select_K%d" % K])
            # the old way's own repeatability: its even rounds against its odd rounds
            own = abs(float(np.median(old[0::2])) - float(np.median(old[1::2]))) if runs > 1 else 0.0
            new = med["neighbors_K%d_ms" % K]
            out["K"][str(K)] = {"neighbors_ms": new, "old_way_ms": float(np.median(old)), "old_way_own_difference_ms": own,
                                "shorter_by_more_than_that": bool(new + own < float(np.median(old))),
                                "below_the_view_alone": bool(new < med["view_ms"])}
        return out
    finally:
        b.close()


# ---- run_ms in a process of its own (this build or, through EDLIB_AMD_LIB, the parent's)

def run_child(a):
    out = {}
    for s in shapes(a):
        if s.name == "self_hits_both":
            continue
        b = s.make()
        try:
            b.run()
            out[s.name] = float(np.median([b.run()["run_ms"] for _ in range(a.runs)]))
        finally:
            b.close()
    print(json.dumps(out))


def run_ms_legs(a):
    def child(lib):
        env = dict(os.environ)
        if lib:
            env["EDLIB_AMD_LIB"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--run-child", "--families", str(a.families),
                            "--amplicons", str(a.amplicons), "--reads", str(a.reads), "--runs", str(a.runs)],
                           env=env, check=True, stdout=subprocess.PIPE)
        return json.loads(p.stdout.decode().strip().splitlines()[-1])
    first = child(None)
    parent = child(a.parent_lib) if a.parent_lib else None
    second = child(None)
    out = {"this_build": [first, second], "parent": parent or {"not_measured": "no --parent-lib"}}
    if parent:
        out["parent_within_own_difference"] = {
            k: bool(min(first[k], second[k]) - abs(first[k] - second[k]) <= parent[k] <= max(first[k], second[k]) + abs(first[k] - second[k]))
            for k in first}
    return out


# ---- the kernels, traced

def trace_child(a):
    for s in shapes(a):
        if s.name not in ("self_hits_forward", "cross_dense"):
            continue
        b = s.make()
        try:
            b.run()
            for _ in range(5):
                b.neighbors(s.Ks[0])
        finally:
            b.close()


def kernel_times(a):
    """average us of the neighbours kernels and the scan's from rocprofv3's kernel stats of a child of its own"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"not_measured": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="neighbors_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
                            sys.executable, os.path.abspath(__file__), "--trace-child", "--families", str(a.families),
                            "--amplicons", str(a.amplicons), "--reads", str(a.reads)],
                           capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"not_measured": "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-300:])}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                m = re.search(r"neighbors_(\w+?)_kernel", name)
                key = m.group(1) if m else ("scan" if "scan" in name.lower() and "rocprim" in name.lower() else None)
                if key:
                    out.setdefault(key, []).append({"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                                    "name": name[:80]})
        out["note"] = ("select: 5 calls on the self hit list (K = %d) and 5 on the dense cross matrix (K = 3) in one average; "
                       "degree, scatter: the self hit list's mirror; scan: every rocPRIM scan kernel of the process, the "
                       "Runs' included" % 10)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=2000, help="families of 100 in the 32 bp shape")
    ap.add_argument("--amplicons", type=int, default=2000)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_neighbors.json"))
    ap.add_argument("--run-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run_child:
        return run_child(a)
    if a.trace_child:
        return trace_child(a)
    res = {"metric": "bench_neighbors", "runs": a.runs, "shapes": {}}
    for s in shapes(a):
        res["shapes"][s.name] = leg(s, a.runs)
        print(s.name, json.dumps(res["shapes"][s.name]["K"]), file=sys.stderr, flush=True)
    res["run_ms"] = run_ms_legs(a)
    res["kernels"] = {"not_measured": "--no-trace"} if a.no_trace else kernel_times(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
