"""Streamed units beside a batch per chunk on one device: the verification step of a seed-and-extend mapper over one
5 Mb synthetic target and `--chunks` (8) chunks of different content, in two shapes --
  reads       262,144 x 150 bp reads, each HW in one 400-base window around its origin, the UNITS view
  candidates  65,536 reads x 4 candidate windows (one true, three random) with a strand each, the BEST view only
Per shape and chunk three legs run one after the other, so that all see the same minutes of the box:
  (a)  the way without set_units: WindowBatch(...), run(), view, close()      -- twice (a1, a2): its own spread
  (b)  one resident batch: set_units(), run(), view
Per leg the per-chunk medians of create-or-set (for (a): create plus close), run and view in ms, their sum, chunks per
second, word_steps (equal in both legs) and whether the views of both legs were equal on every chunk (asserted); per
shape the ratio (a) / (b) of the per-chunk time beside the disagreement of the two (a) legs.  --parent-lib names a
libedlib.so built from the parent commit: leg (a) then runs once more over the same chunks in a child process that loads
that library through EDLIB_AMD_LIB (`a_parent`).  Writes one JSON line to profiles/bench_windows_stream.json and prints
it (DESIGN.md §4i "Streamed units").

    python tools/bench_windows_stream.py [--reads 262144] [--chunks 8] [--parent-lib PATH] [--out profiles/bench_windows_stream.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import edlib_amd  # noqa: E402
from edlib_amd import synth  # noqa: E402

M, W = 150, 400
SHAPES = ("reads", "candidates")


def chunk_of(shape, target, nreads, seed):
    """(queries [n][150], unit_query, unit_start, unit_length, unit_strand or None) of one chunk"""
    n = nreads if shape == "reads" else nreads // 4
    R = synth.illumina_reads(target, n, m=M, seed=seed)
    reads, pos = R["reads"], np.asarray(R["start"], dtype=np.int64)
    start = np.clip(pos - 125, 0, len(target) - W).astype(np.int32)
    if shape == "reads":
        return reads, np.arange(n, dtype=np.int32), start, np.full(n, W, dtype=np.int32), None
    rng = np.random.default_rng(seed)
    flip = rng.integers(0, 2, size=n).astype(bool)       # reads sequenced from the other strand
    reads = np.where(flip[:, None], _revcomp(reads), reads)
    cs = rng.integers(0, len(target) - W + 1, size=(n, 4)).astype(np.int32)
    st = rng.integers(0, 2, size=(n, 4)).astype(np.uint8)
    slot = rng.integers(0, 4, size=n)
    cs[np.arange(n), slot] = start
    st[np.arange(n), slot] = flip
    return (np.ascontiguousarray(reads), np.repeat(np.arange(n, dtype=np.int32), 4), cs.reshape(-1),
            np.full(4 * n, W, dtype=np.int32), st.reshape(-1))


_COMP = np.arange(256, dtype=np.uint8)
_COMP[list(b"ACGTacgt")] = list(b"TGCAtgca")


def _revcomp(reads):
    return _COMP[reads[:, ::-1]]


def view_of(b, shape):
    return b.units(copy=False) if shape == "reads" else b.best(copy=False)


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def leg_a(target, chunk, shape):
    q, uq, us, ul, st = chunk
    b, make_ms = timed(lambda: edlib_amd.WindowBatch(q, target, uq, us, ul, mode="HW", unit_strand=st))
    try:
        stats, run_ms = timed(b.run)
        v, view_ms = timed(lambda: view_of(b, shape))
        v = {f: np.array(x) for f, x in v.items()}
    finally:
        _, close_ms = timed(b.close)
    return {"make_ms": make_ms + close_ms, "run_ms": run_ms, "view_ms": view_ms, "word_steps": stats["word_steps"]}, v


def leg_b(b, chunk, shape):
    q, uq, us, ul, st = chunk
    _, make_ms = timed(lambda: b.set_units(q, uq, us, ul, unit_strand=st))
    stats, run_ms = timed(b.run)
    v, view_ms = timed(lambda: view_of(b, shape))
    return {"make_ms": make_ms, "run_ms": run_ms, "view_ms": view_ms, "word_steps": stats["word_steps"]}, v


def summary(rows):
    out = {f: float(np.median([r[f] for r in rows])) for f in ("make_ms", "run_ms", "view_ms")}
    per_chunk = [r["make_ms"] + r["run_ms"] + r["view_ms"] for r in rows]
    out["chunk_ms"] = float(np.median(per_chunk))
    out["chunk_ms_all"] = [round(x, 3) for x in per_chunk]
    out["chunks_per_s"] = 1e3 / out["chunk_ms"]
    out["word_steps"] = sorted({int(r["word_steps"]) for r in rows})
    return out


def only_leg_a(target, a):
    """the child's job (--only-a): leg (a) over every chunk of every shape with whatever library lib() loads; the
    summaries as one JSON line"""
    out = {}
    for shape in SHAPES:
        rows = []
        leg_a(target, chunk_of(shape, target, a.reads, 99), shape)           # warm-up: code objects, the library's caches
        for c in range(a.chunks):
            rows.append(leg_a(target, chunk_of(shape, target, a.reads, 100 + c), shape)[0])
        out[shape] = summary(rows)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--target", type=int, default=5_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-a", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_windows_stream.json"))
    a = ap.parse_args()
    target = synth.random_dna(12345, a.target)
    if a.only_a:
        return only_leg_a(target, a)
    res = {"metric": "bench_windows_stream", "target": a.target, "reads": a.reads, "read": M, "window": W,
           "chunks": a.chunks, "shapes": {}}
    parent = None
    if a.parent_lib:
        # a process of its own: the library is chosen when it is first loaded
        env = dict(os.environ, EDLIB_AMD_LIB=os.path.abspath(a.parent_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-a", "--reads", str(a.reads), "--chunks",
                            str(a.chunks), "--target", str(a.target)], env=env, check=True, stdout=subprocess.PIPE)
        parent = json.loads(p.stdout.decode().strip().splitlines()[-1])
    for shape in SHAPES:
        rows = {"a1": [], "b": [], "a2": []}
        warm = chunk_of(shape, target, a.reads, 99)
        leg_a(target, warm, shape)
        # the resident batch is created over the target alone: every chunk, the first included, comes by set_units
        empty = np.zeros(0, dtype=np.int32)
        resident = edlib_amd.WindowBatch([], target, empty, empty, empty, mode="HW")
        try:
            leg_b(resident, warm, shape)
            for c in range(a.chunks):
                chunk = chunk_of(shape, target, a.reads, 100 + c)
                r, va = leg_a(target, chunk, shape)
                rows["a1"].append(r)
                r, vb = leg_b(resident, chunk, shape)
                rows["b"].append(r)
                assert sorted(va) == sorted(vb) and all(np.array_equal(va[f], vb[f]) for f in va), (shape, c)
                del vb
                r, _ = leg_a(target, chunk, shape)
                rows["a2"].append(r)
        finally:
            resident.close()
        s = {leg: summary(rs) for leg, rs in rows.items()}
        a_ms = 0.5 * (s["a1"]["chunk_ms"] + s["a2"]["chunk_ms"])
        res["shapes"][shape] = {
            "a1": s["a1"], "b": s["b"], "a2": s["a2"], "views_equal": True,
            "word_steps_equal": s["a1"]["word_steps"] == s["b"]["word_steps"] == s["a2"]["word_steps"],
            "a_over_b": a_ms / max(s["b"]["chunk_ms"], 1e-9),
            "a_legs_disagreement": abs(s["a1"]["chunk_ms"] - s["a2"]["chunk_ms"]) / max(a_ms, 1e-9)}
        if parent:
            res["shapes"][shape]["a_parent"] = parent[shape]
            res["shapes"][shape]["a_over_a_parent"] = a_ms / max(parent[shape]["chunk_ms"], 1e-9)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
