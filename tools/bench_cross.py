"""Cross batches (every query against every target) on one device: resident run ms and view ms (BEST only, then MATRIX)
for the demultiplexing shape (96 x 24 bp barcodes against 1M x 150 bp read heads, HW, k = -1) and the all-against-all
shape (2,000 x 150 bp amplicons, NW), and the same cells through PairBatch at a size both routes hold (96 x 20,000),
with a sample of cells checked against the reference.  Hit-list batches ("hits"): run ms, hits-view ms and numHits of
200,000 x 200,000 32 bp sequences (2,000 families of 100, NW, k = 2), of the 2,000 amplicons at NW k = 8 and of the demux
shape at HW k = 3 (each beside the dense batch's run + MATRIX view), and of 2,000 amplicons of 100-200 bp at NW k = 5
(the length window decides most cells).  Prints one JSON line.

    python tools/bench_cross.py [--reads 1000000] [--amplicons 2000] [--runs 5] [--families 2000]
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


def demux_inputs(rng, nreads, nbc=96, bclen=24, rlen=150):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = rng.choice(acgt, size=(nbc, bclen)).astype(np.uint8)
    reads = rng.choice(acgt, size=(nreads, rlen)).astype(np.uint8)
    which = rng.integers(0, nbc, size=nreads)
    reads[:, 10:10 + bclen] = barcodes[which]
    return barcodes, reads


def amplicons(rng, n, length=150):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = rng.choice(acgt, size=length).astype(np.uint8)
    a = np.tile(base, (n, 1))
    for i in range(n):
        pos = rng.integers(0, length, size=int(rng.integers(0, 12)))
        a[i, pos] = rng.choice(acgt, size=len(pos))
    return a


def time_cross(queries, targets, mode, runs, k=-1):
    b = edlib_amd.CrossBatch(queries, targets, mode=mode, k=k)
    b.run()                                                 # warm-up
    ms, scan = [], []
    for _ in range(runs):
        t = time.perf_counter()
        st = b.run()
        ms.append((time.perf_counter() - t) * 1e3)
        scan.append(st["scan_ms"])
    t = time.perf_counter(); best = b.best(copy=False); best_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter(); mat = b.matrix(copy=False); mat_ms = (time.perf_counter() - t) * 1e3
    out = {"run_ms": float(np.median(ms)), "scan_ms": float(np.median(scan)), "view_best_ms": best_ms,
           "view_matrix_ms": mat_ms, "cells": st["cells"], "word_steps": st["word_steps"], "path": st["path"]}
    return b, out, {k: v.copy() for k, v in mat.items()}, {k: v.copy() for k, v in best.items()}


def time_hits(queries, targets, mode, k, runs):
    """A hit-list batch: median resident run ms (scan ms), then the hits view and the BEST view of the last run."""
    b = edlib_amd.CrossBatch(queries, targets, mode=mode, k=k, hits=True)
    st = b.run()                                            # warm-up (a first run past the list's capacity grows it)
    first_ms = st["run_ms"]
    ms, scan = [], []
    for _ in range(runs):
        t = time.perf_counter()
        st = b.run()
        ms.append((time.perf_counter() - t) * 1e3)
        scan.append(st["scan_ms"])
    t = time.perf_counter(); h = b.hits(copy=False); hits_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter(); b.best(copy=False); best_ms = (time.perf_counter() - t) * 1e3
    out = {"run_ms": float(np.median(ms)), "scan_ms": float(np.median(scan)), "first_run_ms": first_ms,
           "view_hits_ms": hits_ms, "view_best_ms": best_ms, "numHits": int(len(h["query"])),
           "cells": st["cells"], "word_steps": st["word_steps"], "path": st["path"]}
    h = {f: v.copy() for f, v in h.items()}
    b.close()
    return out, h


def families(rng, nfam, kids, length=32):
    """nfam random parents with kids children each at 0-2 substitutions."""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = np.repeat(rng.choice(acgt, size=(nfam, length)).astype(np.uint8), kids, axis=0)
    for p in (0.8, 0.5):
        hit = rng.random(len(seqs)) < p
        pos = rng.integers(0, length, size=len(seqs))
        seqs[hit, pos[hit]] = rng.choice(acgt, size=int(hit.sum()))
    return seqs


def check_hits(queries, targets, mode, k, h, n, rng):
    """Sampled hits against the reference: mismatching editDistance values."""
    from oracle import oracle as O
    nh = len(h["query"])
    if nh == 0:
        return 0
    idx = rng.choice(nh, size=min(n, nh), replace=False)
    t_ = np.searchsorted(h["targetOffsets"], idx, side="right") - 1
    qs = [bytes(queries[int(h["query"][i])]) for i in idx]
    ts = [bytes(targets[int(t)]) for t in t_]

    def pack(s):
        off = np.zeros(len(s) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in s])
        return np.frombuffer(b"".join(s) + b"\0", dtype=np.uint8), off
    qp, qo = pack(qs)
    tp, to = pack(ts)
    r = O.pool_align(qp, qo, tp, to, False, mode, "distance", k)
    return int(np.sum(np.asarray(r["editDistance"]) != h["editDistance"][idx]))


def hits_beside_dense(queries, targets, mode, k, runs, check, rng):
    res, h = time_hits(queries, targets, mode, k, runs)
    b, dense, _, _ = time_cross(queries, targets, mode, runs, k=k)
    b.close()
    res["dense_run_ms"] = dense["run_ms"]
    res["dense_view_matrix_ms"] = dense["view_matrix_ms"]
    res["dense_word_steps"] = dense["word_steps"]
    res["shape"] = [len(queries), len(targets)]
    res["k"] = k
    res["sample_mismatches"] = check_hits(queries, targets, mode, k, h, check, rng)
    return res


def check_sample(queries, targets, mode, mat, n, rng):
    from oracle import oracle as O
    nt, nq = mat["editDistance"].shape
    idx = rng.choice(nt * nq, size=min(n, nt * nq), replace=False)
    t_, q_ = idx // nq, idx % nq
    qs = [queries[q].tobytes() for q in q_]
    ts = [targets[t].tobytes() for t in t_]

    def pack(s):
        off = np.zeros(len(s) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in s])
        return np.frombuffer(b"".join(s), dtype=np.uint8), off
    qp, qo = pack(qs)
    tp, to = pack(ts)
    r = O.pool_align(qp, qo, tp, to, False, mode, "distance", -1)
    return int(np.sum(np.asarray(r["editDistance"]) != mat["editDistance"][t_, q_]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--amplicons", type=int, default=2000)
    ap.add_argument("--pair-reads", type=int, default=20_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--families", type=int, default=2000, help="families of 100 in the 32 bp all-against-all shape")
    ap.add_argument("--no-hits", action="store_true", help="only the dense shapes")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"metric": "bench_cross"}

    bc, reads = demux_inputs(rng, a.reads)
    b, res["demux"], mat, _ = time_cross(bc, reads, "HW", a.runs)
    b.close()
    res["demux"]["shape"] = [len(bc), len(reads)]
    res["demux"]["sample_mismatches"] = check_sample(bc, reads, "HW", mat, a.check, rng)
    del mat

    amp = amplicons(rng, a.amplicons)
    b, res["all_against_all"], mat, _ = time_cross(amp, amp, "NW", a.runs)
    b.close()
    res["all_against_all"]["shape"] = [len(amp), len(amp)]
    res["all_against_all"]["sample_mismatches"] = check_sample(amp, amp, "NW", mat, a.check, rng)

    # the same cells through PairBatch (every byte replicated per cell) at a size both routes hold
    small = reads[:a.pair_reads]
    b, cross_small, mat, _ = time_cross(bc, small, "HW", a.runs)
    b.close()
    qi = np.tile(np.arange(len(bc)), len(small))
    ti = np.repeat(np.arange(len(small)), len(bc))
    p = edlib_amd.PairBatch(bc[qi], small[ti], mode="HW", k=-1)
    p.run()
    ms = []
    for _ in range(a.runs):
        t = time.perf_counter(); p.run(); ms.append((time.perf_counter() - t) * 1e3)
    f = p.results_flat()
    p.close()
    res["pairs_vs_cross"] = {"shape": [len(bc), len(small)], "cross_run_ms": cross_small["run_ms"],
                             "pairs_run_ms": float(np.median(ms)),
                             "speedup": float(np.median(ms)) / max(cross_small["run_ms"], 1e-9),
                             "mismatches": int(np.sum(f["editDistance"] != mat["editDistance"].reshape(-1)))}
    del mat

    if not a.no_hits:
        hits = res["hits"] = {}
        seqs = families(rng, a.families, 100)
        r, h = time_hits(seqs, seqs, "NW", 2, max(1, min(a.runs, 3)))
        r["shape"] = [len(seqs), len(seqs)]
        r["k"] = 2
        r["sample_mismatches"] = check_hits(seqs, seqs, "NW", 2, h, a.check, rng)
        hits["all_against_all_32"] = r
        del h
        hits["amplicons_150"] = hits_beside_dense(amp, amp, "NW", 8, a.runs, a.check, rng)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        var = [bytes(amp[i % len(amp)][:int(n)]) + bytes(rng.choice(acgt, size=max(0, int(n) - 150)))
               for i, n in enumerate(rng.integers(100, 201, size=a.amplicons))]
        hits["amplicons_100_200"] = hits_beside_dense(var, var, "NW", 5, a.runs, a.check, rng)
        hits["demux"] = hits_beside_dense(bc, reads, "HW", 3, a.runs, a.check, rng)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
