"""Pairs gathered from a cross or self batch beside pairs materialised on the host, on one device: the step that follows
a cross batch's distances -- the cells it found go through a resident pair batch for locations or CIGAR paths.  Two
workloads, `--chunks` (8) chunks of different content each:
  barcodes_locations   96 x 24 bp barcodes against streamed chunks (set_targets) of `--reads` (1,000,000) x 150 bp reads,
                       HW hits at k = 3; the pair batch takes cell_windows() of ALL hits, HW, locations
  barcodes_path        the same pairs with paths
  self_nw_path         about 40,000 pairs within k of a self hit list over 250 bp sequences, whole targets, NW, paths
Per workload and chunk three legs run one after the other on the same cells, their order rotating from chunk to chunk:
  (a)   the tuples (cell_windows, or the hit list's index pairs), set_cells(source, tuples), run(), results_flat(copy=False);
        tuples and set are timed separately
  (b)   the windows cut out of the reads on the host (numpy, flat data and offsets), edlibAmdBatchPairsSetPairs, run(),
        results_flat(copy=False); materialisation and set are timed separately
  (b2)  leg (b) once more: what two runs of the same leg differ by is the tool's own noise
Each leg has a resident pair batch of its own.  Per leg the per-chunk medians of tuples / materialise, set, run and view in
ms and the device's run_ms; per workload whether the views of all legs were equal on every chunk (asserted), and the bar of
DESIGN.md §4b "Pairs from a cross batch" as a boolean: (a)'s set below (b)'s set by more than (b) and (b2) differ.  Writes
one JSON line to profiles/bench_pairs_cells.json and prints it.

    python tools/bench_pairs_cells.py [--reads 1000000] [--chunks 8] [--out profiles/bench_pairs_cells.json]
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

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def barcode_chunk(rng, barcodes, n):
    """n reads of 150 bp (2-D uint8), each with one of the barcodes at its 5' end behind 0 to 8 bases, 0 to 3 substitutions"""
    reads = DNA[rng.integers(0, 4, size=(n, 150))]
    which = rng.integers(0, len(barcodes), size=n)
    at = rng.integers(0, 9, size=n)
    b = barcodes[which].copy()
    for _ in range(3):
        hit = rng.random(n) < 0.4
        b[hit, rng.integers(0, 24, size=n)[hit]] = DNA[rng.integers(0, 4, size=int(hit.sum()))]
    reads[np.arange(n)[:, None], at[:, None] + np.arange(24)[None, :]] = b
    return np.ascontiguousarray(reads)


def self_chunk(rng, clusters=727, size=11, m=250):
    """clusters x size sequences of m bases, 0 to 3 substitutions around each cluster's centre: 55 pairs within k a cluster"""
    centres = DNA[rng.integers(0, 4, size=(clusters, m))]
    seqs = np.repeat(centres, size, axis=0)
    n = len(seqs)
    for _ in range(3):
        hit = rng.random(n) < 0.5
        seqs[hit, rng.integers(0, m, size=n)[hit]] = DNA[rng.integers(0, 4, size=int(hit.sum()))]
    return np.ascontiguousarray(seqs[rng.permutation(n)])


def slices(flat, row_len, pt, ps, pl):
    """the windows [ps, ps + pl) of rows pt of a 2-D array given flat: data and offsets, two fancy-indexing calls"""
    off = np.zeros(len(pl) + 1, dtype=np.int64)
    off[1:] = np.cumsum(pl)
    first = pt.astype(np.int64) * row_len + ps
    idx = np.arange(off[-1], dtype=np.int64) + np.repeat(first - off[:-1], pl)
    return np.ascontiguousarray(flat[idx]), off


def leg_a(pb, src, make_tuples):
    tup, tup_ms = timed(make_tuples)
    _, set_ms = timed(lambda: pb.set_cells(src, *tup))
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return {"prepare_ms": tup_ms, "set_ms": set_ms, "run_ms": run_ms, "view_ms": view_ms, "device_run_ms": stats["run_ms"]}, v


def leg_b(pb, make_pairs):
    (qd, qo, td, to), mat_ms = timed(make_pairs)
    n = len(qo) - 1

    def set_pairs():
        if edlib_amd.lib().edlibAmdBatchPairsSetPairs(pb._h, qd.ctypes.data, qo.ctypes.data, td.ctypes.data, to.ctypes.data, n):
            raise RuntimeError(edlib_amd.last_error())
        pb.n = n
    _, set_ms = timed(set_pairs)
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return {"prepare_ms": mat_ms, "set_ms": set_ms, "run_ms": run_ms, "view_ms": view_ms, "device_run_ms": stats["run_ms"]}, v


def summary(rows):
    out = {f: float(np.median([r[f] for r in rows])) for f in ("prepare_ms", "set_ms", "run_ms", "view_ms", "device_run_ms")}
    out["chunk_ms"] = float(np.median([r["prepare_ms"] + r["set_ms"] + r["run_ms"] + r["view_ms"] for r in rows]))
    out["set_ms_all"] = [round(r["set_ms"], 3) for r in rows]
    return out


def same_views(va, vb):
    return sorted(va) == sorted(vb) and all((va[f] is None and vb[f] is None) or np.array_equal(va[f], vb[f]) for f in va)


def run_legs(rows, c, pa, pb, src, make_tuples, make_pairs, what):
    order = (["a", "b", "b2"] * 2)[c % 3:c % 3 + 3]
    views = {}
    for leg in order:
        r, v = leg_a(pa, src, make_tuples) if leg == "a" else leg_b(pb, make_pairs)
        rows[leg].append(r)
        # (every leg's view is copied behind its clock: the resident batches run again)
        views[leg] = {f: None if x is None else np.array(x) for f, x in v.items()}
    for leg in ("b", "b2"):
        assert same_views(views["a"], views[leg]), (what, c, leg)
    return len(views["a"]["editDistance"])


def report(rows, pairs):
    s = {leg: summary(rs) for leg, rs in rows.items()}
    b_set = 0.5 * (s["b"]["set_ms"] + s["b2"]["set_ms"])
    noise = abs(s["b"]["set_ms"] - s["b2"]["set_ms"])
    return {"pairs_per_chunk": pairs, "a": s["a"], "b": s["b"], "b2": s["b2"], "views_equal": True,
            "set_b_over_a": b_set / max(s["a"]["set_ms"], 1e-9), "set_b_legs_differ_ms": noise,
            # the bar: (a)'s set below (b)'s by more than the two (b) legs differ
            "a_set_below_b_set": s["a"]["set_ms"] < b_set - noise,
            "materialise_ms_saved": 0.5 * (s["b"]["prepare_ms"] + s["b2"]["prepare_ms"]) - s["a"]["prepare_ms"],
            "chunk_b_over_a": 0.5 * (s["b"]["chunk_ms"] + s["b2"]["chunk_ms"]) / max(s["a"]["chunk_ms"], 1e-9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pairs_cells.json"))
    a = ap.parse_args()
    res = {"metric": "bench_pairs_cells", "reads": a.reads, "chunks": a.chunks, "workloads": {}}
    rng = np.random.default_rng(4242)

    # ---- barcodes against streamed reads
    barcodes = DNA[rng.integers(0, 4, size=(96, 24))]
    qlen, tlen = np.full(96, 24), np.full(a.reads, 150)
    src = edlib_amd.CrossBatch(barcodes, barcode_chunk(rng, barcodes, a.reads), mode="HW", k=3, hits=True)
    batches = {task: (edlib_amd.PairBatch([], [], mode="HW", task=task), edlib_amd.PairBatch([], [], mode="HW", task=task))
               for task in ("locations", "path")}
    rows = {task: {"a": [], "b": [], "b2": []} for task in batches}
    pairs = {task: [] for task in batches}
    try:
        for c in range(-1, a.chunks):                           # chunk -1: warm-up (code objects, the batches' buffers)
            reads = barcode_chunk(rng, barcodes, a.reads)
            flat = reads.reshape(-1)
            src.set_targets(reads)
            src.run()
            hits = src.hits()
            target = np.repeat(np.arange(a.reads), np.diff(hits["targetOffsets"]))

            def make_tuples():
                return edlib_amd.cell_windows("HW", hits["query"], target, hits["editDistance"], hits["endLocation"], qlen,
                                              tlen)[1:]

            def make_pairs():
                _, pq, pt, ps, pl, _ = edlib_amd.cell_windows("HW", hits["query"], target, hits["editDistance"],
                                                              hits["endLocation"], qlen, tlen)
                td, to = slices(flat, 150, pt, ps, pl)
                return np.ascontiguousarray(barcodes[pq]).reshape(-1), np.arange(len(pq) + 1, dtype=np.int64) * 24, td, to

            for task, (pa, pb) in batches.items():
                scratch = {"a": [], "b": [], "b2": []} if c < 0 else rows[task]
                n = run_legs(scratch, max(c, 0), pa, pb, src, make_tuples, make_pairs, task)
                if c >= 0:
                    pairs[task].append(n)
    finally:
        for pa, pb in batches.values():
            pa.close()
            pb.close()
        src.close()
    for task in batches:
        res["workloads"]["barcodes_" + task] = report(rows[task], int(np.median(pairs[task])))

    # ---- the pairs within k of a self hit list, whole sequences
    rows, pairs = {"a": [], "b": [], "b2": []}, []
    pa, pb = edlib_amd.PairBatch([], [], mode="NW", task="path"), edlib_amd.PairBatch([], [], mode="NW", task="path")
    try:
        for c in range(-1, a.chunks):
            seqs = self_chunk(rng)
            src = edlib_amd.SelfBatch(seqs, k=8, hits=True)
            try:
                src.run()
                hits = src.hits()

                def make_tuples():
                    first = np.repeat(np.arange(len(seqs), dtype=np.int32), np.diff(hits["rowOffsets"]))
                    return first, hits["partner"]

                def make_pairs():
                    first, partner = make_tuples()
                    off = np.arange(len(first) + 1, dtype=np.int64) * 250
                    return np.ascontiguousarray(seqs[first]).reshape(-1), off, np.ascontiguousarray(seqs[partner]).reshape(-1), off

                n = run_legs({"a": [], "b": [], "b2": []} if c < 0 else rows, max(c, 0), pa, pb, src, make_tuples, make_pairs,
                             "self")
                if c >= 0:
                    pairs.append(n)
            finally:
                src.close()
    finally:
        pa.close()
        pb.close()
    res["workloads"]["self_nw_path"] = report(rows, int(np.median(pairs)))

    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
