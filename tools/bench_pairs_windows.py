"""Pairs gathered from a window batch beside pairs materialised on the host, on one device: the step of a mapper's loop
that follows the verification -- a streamed window batch has run over the chunk's reads and candidate windows, and the
winners now go through a resident pair batch for distances or CIGAR paths -- `--chunks` (8) chunks of different content,
in three shapes over a 5 Mb target, half of the reads from the reverse strand --
  hw_distance   262,144 x (150 bp read in a 400-base window), HW, distance
  hw_path       the same pairs with paths
  nw_path_250   40,000 x (250 bp read in its 250-base window), NW, paths: the bases of 10,000 x 1 kb, the shape where
                set_pairs brought no gain, as units a window batch prepares on the device (queries of at most 256 bases;
                1 kb queries are out of set_windows' reach, see `nw_path_1kb`)
Per shape and chunk three legs run one after the other on the same tuples, their order rotating from chunk to chunk:
  (a)   set_windows(window batch, tuples), run(), results_flat(copy=False)
  (b)   the slices cut out of the target and the strand-1 reads reverse-complemented on the host (numpy), set_pairs(),
        run(), results_flat(copy=False); materialisation and set are timed separately
  (b2)  leg (b) once more: what two runs of the same leg differ by is the tool's own noise
Each leg has a resident pair batch of its own kind.  Per leg the per-chunk medians of materialise, set, run and view in ms
and the device's run_ms; per shape whether the views of all legs were equal on every chunk (asserted), and the bar of
DESIGN.md §4b "Pairs from a window batch" as booleans: (a)'s set below (b)'s set by more than (b) and (b2) differ, and
(a)'s device run_ms within that same kind of noise of (b)'s.  Writes one JSON line to profiles/bench_pairs_windows.json
and prints it.

    python tools/bench_pairs_windows.py [--pairs 262144] [--chunks 8] [--out profiles/bench_pairs_windows.json]
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
from edlib_amd import synth  # noqa: E402

SHAPES = {"hw_distance": ("HW", "distance", 150, 400), "hw_path": ("HW", "path", 150, 400),
          "nw_path_250": ("NW", "path", 250, 250)}
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def chunk_of(shape, genome, npairs, seed):
    """the reads of one chunk as the sequencer gave them (2-D uint8; the odd ones come from the reverse strand), and per
    read the window it is verified in: start, length, strand"""
    _, _, m, w = SHAPES[shape]
    n = npairs if m == 150 else max(npairs * 40000 // 262144, 1)
    R = synth.illumina_reads(genome, n, m=m, seed=seed)
    reads = np.ascontiguousarray(R["reads"])
    strand = (np.arange(n) & 1).astype(np.uint8)
    reads[1::2] = COMP[reads[1::2, ::-1]]
    start = np.clip(np.asarray(R["start"], dtype=np.int64) - (w - m) // 2, 0, len(genome) - w).astype(np.int32)
    return reads, start, np.full(n, w, dtype=np.int32), strand


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def _row(mat_ms, set_ms, run_ms, view_ms, stats):
    return {"materialise_ms": mat_ms, "set_ms": set_ms, "run_ms": run_ms, "view_ms": view_ms,
            "device_run_ms": stats["run_ms"], "word_steps": stats["word_steps"]}


def leg_a(pb, wb, tuples):
    _, set_ms = timed(lambda: pb.set_windows(wb, *tuples))
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return _row(0.0, set_ms, run_ms, view_ms, stats), v


def materialise(genome, reads, start, length, strand):
    """what a caller does without set_windows: every window cut out of the target, the reads of strand 1 reversed and
    complemented (windows of one length: two fancy-indexing calls)"""
    windows = genome[start.astype(np.int64)[:, None] + np.arange(int(length[0]))[None, :]]
    q = reads.copy()
    rev = strand.astype(bool)
    q[rev] = COMP[q[rev, ::-1]]
    return np.ascontiguousarray(q), np.ascontiguousarray(windows)


def leg_b(pb, genome, reads, start, length, strand):
    (q, t), mat_ms = timed(lambda: materialise(genome, reads, start, length, strand))
    _, set_ms = timed(lambda: pb.set_pairs(q, t))
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return _row(mat_ms, set_ms, run_ms, view_ms, stats), v


def summary(rows):
    out = {f: float(np.median([r[f] for r in rows])) for f in ("materialise_ms", "set_ms", "run_ms", "view_ms", "device_run_ms")}
    per_chunk = [r["materialise_ms"] + r["set_ms"] + r["run_ms"] + r["view_ms"] for r in rows]
    out["chunk_ms"] = float(np.median(per_chunk))
    out["set_ms_all"] = [round(r["set_ms"], 3) for r in rows]
    out["device_run_ms_all"] = [round(r["device_run_ms"], 4) for r in rows]
    out["word_steps"] = sorted({int(r["word_steps"]) for r in rows})
    return out


def same_views(va, vb):
    return sorted(va) == sorted(vb) and all((va[f] is None and vb[f] is None) or np.array_equal(va[f], vb[f]) for f in va)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=262144)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pairs_windows.json"))
    a = ap.parse_args()
    genome = synth.random_dna(12345, a.genome)
    res = {"metric": "bench_pairs_windows", "pairs": a.pairs, "chunks": a.chunks, "genome": a.genome, "shapes": {},
           "nw_path_1kb": "out of reach: set_windows names whole queries of the window batch, and a set a window batch "
                          "prepares on the device holds queries of at most 256 bases; nw_path_250 has the same bases"}
    for shape, (mode, task, m, w) in SHAPES.items():
        rows = {"a": [], "b": [], "b2": []}
        reads, start, length, strand = chunk_of(shape, genome, a.pairs, 99)
        n = len(reads)
        unit_query = np.arange(n, dtype=np.int32)
        # the verification stage: one stranded window batch, every chunk's reads and units by set_units
        wb = edlib_amd.WindowBatch(reads, genome, unit_query, start, length, mode=mode, unit_strand=strand)
        pa = edlib_amd.PairBatch([], [], mode=mode, task=task)
        pb = edlib_amd.PairBatch([], [], mode=mode, task=task)
        try:
            wb.run()
            leg_a(pa, wb, (unit_query, start, length, strand))             # warm-up: code objects, the batches' buffers
            leg_b(pb, genome, reads, start, length, strand)
            for c in range(a.chunks):
                reads, start, length, strand = chunk_of(shape, genome, a.pairs, 100 + c)
                wb.set_units(reads, unit_query, start, length, unit_strand=strand)
                wb.run()
                wb.best(copy=False)
                order = (["a", "b", "b2"] * 2)[c % 3:c % 3 + 3]
                views = {}
                for leg in order:
                    r, v = (leg_a(pa, wb, (unit_query, start, length, strand)) if leg == "a"
                            else leg_b(pb, genome, reads, start, length, strand))
                    rows[leg].append(r)
                    # (every leg's view is copied behind its clock: the resident batches run again)
                    views[leg] = {f: None if x is None else np.array(x) for f, x in v.items()}
                for leg in ("b", "b2"):
                    assert same_views(views["a"], views[leg]), (shape, c, leg)
                del views
        finally:
            pa.close()
            pb.close()
            wb.close()
        s = {leg: summary(rs) for leg, rs in rows.items()}
        b_set = 0.5 * (s["b"]["set_ms"] + s["b2"]["set_ms"])
        set_noise = abs(s["b"]["set_ms"] - s["b2"]["set_ms"])
        b_run = 0.5 * (s["b"]["device_run_ms"] + s["b2"]["device_run_ms"])
        run_noise = abs(s["b"]["device_run_ms"] - s["b2"]["device_run_ms"])
        res["shapes"][shape] = {
            "n": n, "read": m, "window": w, "a": s["a"], "b": s["b"], "b2": s["b2"], "views_equal": True,
            "word_steps_equal": s["a"]["word_steps"] == s["b"]["word_steps"] == s["b2"]["word_steps"],
            "set_b_over_a": b_set / max(s["a"]["set_ms"], 1e-9),
            "set_b_legs_differ_ms": set_noise,
            # the bar: (a)'s set below (b)'s by more than the two (b) legs differ
            "a_set_below_b_set": s["a"]["set_ms"] < b_set - set_noise,
            "materialise_ms_saved": 0.5 * (s["b"]["materialise_ms"] + s["b2"]["materialise_ms"]),
            "device_run_b_legs_differ_ms": run_noise,
            "device_run_a_minus_b_ms": s["a"]["device_run_ms"] - b_run,
            "a_run_within_noise": abs(s["a"]["device_run_ms"] - b_run) <= run_noise,
            "chunk_b_over_a": 0.5 * (s["b"]["chunk_ms"] + s["b2"]["chunk_ms"]) / max(s["a"]["chunk_ms"], 1e-9)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
