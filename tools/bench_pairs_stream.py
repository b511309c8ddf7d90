"""Streamed pairs beside a batch per chunk on one device: the second step of a pipeline that verified with a streamed
window or cross batch and now fetches distances, or start locations and CIGAR paths, for the winners -- `--chunks` (8)
chunks of different content, in three shapes --
  hw_distance   262,144 x (150 bp read in a 400-base window), HW, distance
  hw_path       the same pairs with paths
  nw_path_1kb   10,000 x 1 kb, NW, paths (config 5's shape)
Per shape and chunk three legs run one after the other, so that all see the same minutes of the box:
  (a)  the way without set_pairs: PairBatch(...), run(), results_flat(copy=False), close()   -- twice (a1, a2): its spread
  (b)  one resident batch, created over zero pairs: set_pairs(), run(), results_flat(copy=False)
The order of the three rotates from chunk to chunk (a1 b a2, b a2 a1, a2 a1 b, ...), so that what a leg's place in the
chunk costs -- the first leg runs behind the host's generation of the chunk, the later ones behind a leg's 40 MB copy of
its view -- falls on every leg alike; `by_position` has the medians of run and view by place, whatever leg stood there.
Per leg the per-chunk medians of create-or-set (for (a): create plus close), run and view in ms, their sum, the device's
own run_ms, word_steps (equal in both legs), and whether the views of both legs were equal on every chunk (asserted); per
shape the ratio (a) / (b) of the per-chunk time beside the disagreement of the two (a) legs, and the bar of DESIGN.md §4b
"Streamed pairs" as booleans: whole chunks against the difference of the (a) legs' chunk times, device run_ms and view_ms
each against the difference of the (a) legs in that same figure.  --parent-lib names a libedlib.so built from the parent
commit: leg (a) then runs over the same chunks in a child process that loads that library through EDLIB_AMD_LIB
(`a_parent`), and in another child with this build's library (`a_child`): like beside like.  Writes one JSON line to
profiles/bench_pairs_stream.json and prints it.

    python tools/bench_pairs_stream.py [--pairs 262144] [--chunks 8] [--parent-lib PATH] [--out profiles/bench_pairs_stream.json]
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

M, W, KB = 150, 400, 1000
SHAPES = {"hw_distance": ("HW", "distance"), "hw_path": ("HW", "path"), "nw_path_1kb": ("NW", "path")}
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def chunk_of(shape, genome, npairs, seed):
    """(queries, targets) of one chunk, as 2-D uint8 arrays"""
    if shape == "nw_path_1kb":
        n = max(npairs * 10000 // 262144, 1)
        t = synth.random_dna(seed, n * KB).reshape(n, KB)
        q = t.copy()
        hit = synth.rand_unit(seed, n * KB, stream=1).reshape(n, KB) < 0.04
        other = synth.random_dna(seed, n * KB, stream=2).reshape(n, KB)
        q[hit] = other[hit]
        return np.ascontiguousarray(q), np.ascontiguousarray(t)
    R = synth.illumina_reads(genome, npairs, m=M, seed=seed)
    start = np.clip(np.asarray(R["start"], dtype=np.int64) - 125, 0, len(genome) - W)
    windows = genome[start[:, None] + np.arange(W)[None, :]]
    return np.ascontiguousarray(R["reads"]), np.ascontiguousarray(windows)


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def _row(make_ms, run_ms, view_ms, stats):
    return {"make_ms": make_ms, "run_ms": run_ms, "view_ms": view_ms, "device_run_ms": stats["run_ms"],
            "word_steps": stats["word_steps"]}


def leg_a(chunk, shape):
    mode, task = SHAPES[shape]
    b, make_ms = timed(lambda: edlib_amd.PairBatch(chunk[0], chunk[1], mode=mode, task=task))
    try:
        stats, run_ms = timed(b.run)
        v, view_ms = timed(lambda: b.results_flat(copy=False))
        v = {f: None if x is None else np.array(x) for f, x in v.items()}
    finally:
        _, close_ms = timed(b.close)
    return _row(make_ms + close_ms, run_ms, view_ms, stats), v


def leg_b(b, chunk):
    _, make_ms = timed(lambda: b.set_pairs(chunk[0], chunk[1]))
    stats, run_ms = timed(b.run)
    v, view_ms = timed(lambda: b.results_flat(copy=False))
    return _row(make_ms, run_ms, view_ms, stats), v


def summary(rows):
    out = {f: float(np.median([r[f] for r in rows])) for f in ("make_ms", "run_ms", "view_ms", "device_run_ms")}
    per_chunk = [r["make_ms"] + r["run_ms"] + r["view_ms"] for r in rows]
    out["chunk_ms"] = float(np.median(per_chunk))
    out["chunk_ms_all"] = [round(x, 3) for x in per_chunk]
    out["word_steps"] = sorted({int(r["word_steps"]) for r in rows})
    return out


def only_leg_a(genome, a):
    """the child's job (--only-a): leg (a) over every chunk of every shape with whatever library lib() loads; the
    summaries as one JSON line"""
    out = {}
    for shape in SHAPES:
        leg_a(chunk_of(shape, genome, a.pairs, 99), shape)                  # warm-up: code objects, the library's caches
        rows = [leg_a(chunk_of(shape, genome, a.pairs, 100 + c), shape)[0] for c in range(a.chunks)]
        out[shape] = summary(rows)
    print(json.dumps(out))


def same_views(va, vb):
    return sorted(va) == sorted(vb) and all((va[f] is None and vb[f] is None) or np.array_equal(va[f], vb[f]) for f in va)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=262144)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-a", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pairs_stream.json"))
    a = ap.parse_args()
    genome = synth.random_dna(12345, a.genome)
    if a.only_a:
        return only_leg_a(genome, a)
    res = {"metric": "bench_pairs_stream", "pairs": a.pairs, "read": M, "window": W, "chunks": a.chunks, "shapes": {}}
    parent = child = None
    if a.parent_lib:
        # processes of their own: the library is chosen when it is first loaded.  This build's runs between two of the parent's
        def only_a(lib):
            env = dict(os.environ)
            env.pop("EDLIB_AMD_LIB", None)
            if lib:
                env["EDLIB_AMD_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-a", "--pairs", str(a.pairs), "--chunks",
                                str(a.chunks), "--genome", str(a.genome)], env=env, check=True, stdout=subprocess.PIPE)
            return json.loads(p.stdout.decode().strip().splitlines()[-1])
        parent, child, parent2 = only_a(a.parent_lib), only_a(None), only_a(a.parent_lib)
    for shape, (mode, task) in SHAPES.items():
        rows = {"a1": [], "b": [], "a2": []}
        warm = chunk_of(shape, genome, a.pairs, 99)
        leg_a(warm, shape)
        # the resident batch is created over zero pairs: every chunk, the first included, comes by set_pairs
        resident = edlib_amd.PairBatch([], [], mode=mode, task=task)
        try:
            leg_b(resident, warm)
            place = [[], [], []]
            for c in range(a.chunks):
                chunk = chunk_of(shape, genome, a.pairs, 100 + c)
                order = (["a1", "b", "a2"] * 2)[c % 3:c % 3 + 3]
                views = {}
                for at, leg in enumerate(order):
                    r, v = leg_b(resident, chunk) if leg == "b" else leg_a(chunk, shape)
                    rows[leg].append(r)
                    place[at].append(r)
                    # (every leg's view is copied behind its clock: leg (a)'s batch is gone, the resident one runs again)
                    views[leg] = {f: None if x is None else np.array(x) for f, x in v.items()}
                for leg in ("a1", "a2"):
                    assert same_views(views[leg], views["b"]), (shape, c, leg)
                del views
        finally:
            resident.close()
        s = {leg: summary(rs) for leg, rs in rows.items()}
        a_ms = 0.5 * (s["a1"]["chunk_ms"] + s["a2"]["chunk_ms"])
        noise_ms = abs(s["a1"]["chunk_ms"] - s["a2"]["chunk_ms"])
        a_run = 0.5 * (s["a1"]["device_run_ms"] + s["a2"]["device_run_ms"])
        run_noise = abs(s["a1"]["device_run_ms"] - s["a2"]["device_run_ms"])
        a_view = 0.5 * (s["a1"]["view_ms"] + s["a2"]["view_ms"])
        view_noise = abs(s["a1"]["view_ms"] - s["a2"]["view_ms"])
        out = {"n": int(len(warm[0])), "a1": s["a1"], "b": s["b"], "a2": s["a2"], "views_equal": True,
               "word_steps_equal": s["a1"]["word_steps"] == s["b"]["word_steps"] == s["a2"]["word_steps"],
               "a_over_b": a_ms / max(s["b"]["chunk_ms"], 1e-9),
               "a_legs_differ_ms": noise_ms, "a_legs_disagreement": noise_ms / max(a_ms, 1e-9),
               # the bar: (b) below (a) by more than the (a) legs differ; a streamed Run does not pay for the streaming
               "b_below_a": s["b"]["chunk_ms"] < a_ms - noise_ms,
               "device_run_legs_differ_ms": run_noise, "view_legs_differ_ms": view_noise,
               "streamed_run_within_noise": s["b"]["device_run_ms"] - a_run <= run_noise,
               "streamed_view_within_noise": s["b"]["view_ms"] - a_view <= view_noise,
               "by_position": [{f: float(np.median([r[f] for r in rs])) for f in ("make_ms", "run_ms", "view_ms", "device_run_ms")}
                               for rs in place]}
        if parent:
            out["a_parent"], out["a_child"], out["a_parent2"] = parent[shape], child[shape], parent2[shape]
            # ... and Create did not get slower: this build's child between the parent's two, whose difference is the noise
            p_ms = 0.5 * (parent[shape]["chunk_ms"] + parent2[shape]["chunk_ms"])
            p_run = 0.5 * (parent[shape]["device_run_ms"] + parent2[shape]["device_run_ms"])
            out["a_child_over_a_parent"] = child[shape]["chunk_ms"] / max(p_ms, 1e-9)
            out["parent_legs_differ_ms"] = abs(parent[shape]["chunk_ms"] - parent2[shape]["chunk_ms"])
            out["parent_device_run_legs_differ_ms"] = abs(parent[shape]["device_run_ms"] - parent2[shape]["device_run_ms"])
            out["a_within_noise_of_parent"] = child[shape]["chunk_ms"] - p_ms <= out["parent_legs_differ_ms"]
            out["a_run_within_noise_of_parent"] = child[shape]["device_run_ms"] - p_run <= out["parent_device_run_legs_differ_ms"]
        res["shapes"][shape] = out
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
