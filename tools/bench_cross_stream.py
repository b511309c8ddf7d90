"""Streamed targets beside a batch per chunk on one device: the demultiplexing shape (96 x 24 bp barcodes, HW) over
`--chunks` (8) chunks of 1M x 150 bp reads of different content, as three kinds of cross batch -- dense with the BEST view
only, hit list at k = 3, occurrences at k = 3.  Per kind and chunk three legs run one after the other, so that all see
the same minutes of the box:
  (a)  the way without set_targets: CrossBatch(...), run(), view, close()      -- twice (a1, a2): its own spread
  (b)  one resident batch: set_targets(), run(), view
Per leg the per-chunk medians of create-or-set (for (a): create plus close), run and view in ms, their sum, chunks per
second, word_steps (equal in both legs) and whether the views of both legs were equal on every chunk; per kind the
ratio (a) / (b) of the per-chunk time beside the disagreement of the two (a) legs.  Writes one JSON line to
profiles/bench_cross_stream.json and prints it (DESIGN.md §4h "Streamed targets").

    python tools/bench_cross_stream.py [--reads 1000000] [--chunks 8] [--k 3] [--out profiles/bench_cross_stream.json]
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

KINDS = {"dense_best": dict(), "hits": dict(hits=True), "occurrences": dict(occurrences=True)}


def chunk_of_reads(rng, barcodes, nreads, rlen=150):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = acgt[rng.integers(0, 4, size=(nreads, rlen), dtype=np.uint8)]
    nbc, bclen = barcodes.shape
    reads[:, 10:10 + bclen] = barcodes[rng.integers(0, nbc, size=nreads)]
    return reads


def view_of(b, kind):
    if kind == "dense_best":
        return b.best(copy=False)
    return b.occurrences(copy=False) if kind == "occurrences" else b.hits(copy=False)


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def leg_a(barcodes, reads, kind, k):
    b, make_ms = timed(lambda: edlib_amd.CrossBatch(barcodes, reads, mode="HW", k=k, **KINDS[kind]))
    try:
        st, run_ms = timed(b.run)
        v, view_ms = timed(lambda: view_of(b, kind))
        v = {f: np.array(x) for f, x in v.items()}
    finally:
        _, close_ms = timed(b.close)
    return {"make_ms": make_ms + close_ms, "run_ms": run_ms, "view_ms": view_ms, "word_steps": st["word_steps"]}, v


def leg_b(b, reads, kind):
    _, make_ms = timed(lambda: b.set_targets(reads))
    st, run_ms = timed(b.run)
    v, view_ms = timed(lambda: view_of(b, kind))
    return {"make_ms": make_ms, "run_ms": run_ms, "view_ms": view_ms, "word_steps": st["word_steps"]}, v


def summary(rows):
    out = {f: float(np.median([r[f] for r in rows])) for f in ("make_ms", "run_ms", "view_ms")}
    per_chunk = [r["make_ms"] + r["run_ms"] + r["view_ms"] for r in rows]
    out["chunk_ms"] = float(np.median(per_chunk))
    out["chunk_ms_all"] = [round(x, 3) for x in per_chunk]
    out["chunks_per_s"] = 1e3 / out["chunk_ms"]
    out["word_steps"] = sorted({int(r["word_steps"]) for r in rows})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_cross_stream.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = acgt[rng.integers(0, 4, size=(96, 24), dtype=np.uint8)]
    chunks = [chunk_of_reads(rng, barcodes, a.reads) for _ in range(a.chunks)]
    res = {"metric": "bench_cross_stream", "shape": [len(barcodes), a.reads], "chunks": a.chunks, "k": a.k, "kinds": {}}
    for kind in KINDS:
        k = -1 if kind == "dense_best" else a.k
        rows = {"a1": [], "b": [], "a2": []}
        equal = True
        # the resident batch starts on a few reads of its own: every chunk, the first included, comes by set_targets
        resident = edlib_amd.CrossBatch(barcodes, chunks[0][:64], mode="HW", k=k, **KINDS[kind])
        try:
            for reads in chunks:
                r, va = leg_a(barcodes, reads, kind, k)
                rows["a1"].append(r)
                r, vb = leg_b(resident, reads, kind)
                rows["b"].append(r)
                equal = equal and sorted(va) == sorted(vb) and all(np.array_equal(va[f], vb[f]) for f in va)
                del vb
                r, _ = leg_a(barcodes, reads, kind, k)
                rows["a2"].append(r)
        finally:
            resident.close()
        s = {leg: summary(rs) for leg, rs in rows.items()}
        a_ms = 0.5 * (s["a1"]["chunk_ms"] + s["a2"]["chunk_ms"])
        res["kinds"][kind] = {
            "a1": s["a1"], "b": s["b"], "a2": s["a2"], "views_equal": bool(equal),
            "word_steps_equal": s["a1"]["word_steps"] == s["b"]["word_steps"] == s["a2"]["word_steps"],
            "a_over_b": a_ms / max(s["b"]["chunk_ms"], 1e-9),
            "a_legs_disagreement": abs(s["a1"]["chunk_ms"] - s["a2"]["chunk_ms"]) / max(a_ms, 1e-9)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
