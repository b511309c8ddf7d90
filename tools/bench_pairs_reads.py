"""Pairs gathered from a read batch beside pairs materialised on the host, on one device: the step that follows a
mapper's distance Run -- a read batch has mapped the chunk's reads against the whole target, and the first hit of every
read that mapped now goes through a resident pair batch for start locations and CIGAR paths -- `--chunks` (8) chunks of
different content, in three shapes over a 5 Mb target, reads at 2 % substitutions --
  hw_distance   262,144 x 150 bp, half of them from the reverse strand, out of a BothStrandsBatch (HW, distance, k = 15);
                the pair batch HW, distance
  hw_path       the same with the pair batch HW, path
  nw_path_250   40,000 x 250 bp out of a SharedBatch (HW, distance, k = 25); the pair batch NW, path
The tuples of a chunk are first_hit_windows() of the read batch's results: the window [max(0, e - m - d + 1), e] of every
read with a hit.  Per shape and chunk the legs run one after the other on the same tuples, their order rotating from
chunk to chunk:
  (a)   first_hit_windows() + set_shared_windows(read batch, tuples), run(), results_flat(copy=False)
  (b)   the windows cut out of the target and the strand-1 reads reverse-complemented on the host (numpy), SetPairs, run(),
        results_flat(copy=False); materialisation and set are timed separately
  (b2)  leg (b) once more: what two runs of the same leg differ by is the tool's own noise
  (w)   set_windows() from a window batch over the same target, reads and tuples: the gather from the 4-bit pack beside
        the gather from the raw bytes, like for like
  (d)   reported only: the distance Run that every leg follows, run() + results_flat(copy=False)
  (c)   reported only: a read batch of the same kind with task="path" over the same chunk, run() + results_flat(): what
        it takes beyond (d) is the price of paths inside the read batch, beside (a)'s whole chunk
Each leg has a resident pair batch of its own.  The views of (a), (b), (b2) and (w) must be equal on every chunk
(asserted); where the pair batch is HW the distance and first end of (a), shifted by the window's start, must equal
(c)'s, and with paths the first start and the alignment, too (asserted).  Per leg the per-chunk medians of tuples /
materialise, set, run and view in ms and the device's run_ms; per shape the bars of DESIGN.md §4b "Pairs from a read
batch" as booleans: (a)'s set below (b)'s set by more than (b) and (b2) differ, and (a)'s device run_ms within that same
kind of noise of (b)'s.  Writes one JSON line to profiles/bench_pairs_reads.json and prints it.

    python tools/bench_pairs_reads.py [--pairs 262144] [--chunks 8] [--shapes hw_distance,hw_path,nw_path_250]
                                      [--out profiles/bench_pairs_reads.json]
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

# shape: source kind, the pair batch's mode and task, read length, k of the distance Run
SHAPES = {"hw_distance": ("both", "HW", "distance", 150, 15), "hw_path": ("both", "HW", "path", 150, 15),
          "nw_path_250": ("shared", "NW", "path", 250, 25)}
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def chunk_of(shape, genome, npairs, seed):
    """the reads of one chunk as the sequencer gave them (2-D uint8; from both strands the odd ones come from the reverse
    strand)"""
    kind, _, _, m, _ = SHAPES[shape]
    n = npairs if m == 150 else max(npairs * 40000 // 262144, 1)
    reads = np.ascontiguousarray(synth.illumina_reads(genome, n, m=m, seed=seed, sub=0.02)["reads"])
    if kind == "both":
        reads[1::2] = COMP[reads[1::2, ::-1]]
    return reads


def read_batch(shape, reads, genome, task):
    kind, _, _, _, k = SHAPES[shape]
    cls = edlib_amd.BothStrandsBatch if kind == "both" else edlib_amd.SharedBatch
    return cls(reads, genome, mode="HW", task=task, k=k)


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def _row(mat_ms, set_ms, run_ms, view_ms, stats):
    return {"materialise_ms": mat_ms, "set_ms": set_ms, "run_ms": run_ms, "view_ms": view_ms,
            "device_run_ms": stats["run_ms"], "word_steps": stats["word_steps"]}


def tuples_of(rb, m):
    """the first hit of every read of a read batch that has run"""
    flat = rb.results_flat(copy=False)
    strand = rb.strands(copy=False)[0] if isinstance(rb, edlib_amd.BothStrandsBatch) else None
    return edlib_amd.first_hit_windows(flat, np.full(rb.n, m), strand)


def leg_a(pb, rb, m):
    tup, tup_ms = timed(lambda: tuples_of(rb, m))
    _, set_ms = timed(lambda: pb.set_shared_windows(rb, *tup))
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return _row(tup_ms, set_ms, run_ms, view_ms, stats), v


def leg_w(pb, wb, tup):
    _, set_ms = timed(lambda: pb.set_windows(wb, *tup))
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return _row(0.0, set_ms, run_ms, view_ms, stats), v


def materialise(genome, reads, tup):
    """what a caller does without set_shared_windows: every window cut out of the target (windows of their own lengths:
    one flat index), the reads of strand 1 reversed and complemented"""
    read, start, length, strand = tup
    toff = np.zeros(len(read) + 1, dtype=np.int64)
    toff[1:] = np.cumsum(length)
    idx = np.arange(toff[-1]) + np.repeat(start.astype(np.int64) - toff[:-1], length)
    windows = genome[idx]
    q = reads[read]
    if strand is not None:
        rev = strand.astype(bool)
        q[rev] = COMP[q[rev, ::-1]]
    qoff = np.arange(len(read) + 1, dtype=np.int64) * reads.shape[1]
    return np.ascontiguousarray(q).reshape(-1), qoff, np.ascontiguousarray(windows), toff


def leg_b(pb, genome, reads, rb, m):
    def mat():
        return materialise(genome, reads, tuples_of(rb, m))

    def set_pairs(q, qoff, t, toff):
        if edlib_amd.lib().edlibAmdBatchPairsSetPairs(pb._h, q.ctypes.data, qoff.ctypes.data, t.ctypes.data, toff.ctypes.data,
                                                      len(qoff) - 1) != 0:
            raise RuntimeError(edlib_amd.last_error())
        pb.n = len(qoff) - 1

    pools, mat_ms = timed(mat)
    _, set_ms = timed(lambda: set_pairs(*pools))
    stats, run_ms = timed(pb.run)
    v, view_ms = timed(lambda: pb.results_flat(copy=False))
    return _row(mat_ms, set_ms, run_ms, view_ms, stats), v


def leg_c(shape, reads, genome):
    """the read batch itself with paths: its creation is not timed (the distance batch's is not either)"""
    rc = read_batch(shape, reads, genome, "path")
    try:
        stats, run_ms = timed(rc.run)
        v, view_ms = timed(lambda: rc.results_flat(copy=False))
        v = {f: None if x is None else np.array(x) for f, x in v.items()}
    finally:
        rc.close()
    return {"run_ms": run_ms, "view_ms": view_ms, "device_run_ms": stats["run_ms"]}, v


def first_hits_equal(va, tup, vc, paths):
    """distance, first end (and with paths first start and alignment) of (a), shifted by the window's start, against the
    read batch's own path results for the same reads"""
    read, start = tup[0].astype(np.int64), tup[1].astype(np.int64)
    la, lc = va["locOff"][:-1], vc["locOff"][:-1][read]
    ok = np.array_equal(va["editDistance"], vc["editDistance"][read])
    ok = ok and np.array_equal(va["ends"][la] + start, vc["ends"][lc])
    if paths:
        ok = ok and np.array_equal(va["starts"][la] + start, vc["starts"][lc])
        na, nc = np.diff(va["alnOff"]), np.diff(vc["alnOff"])[read]
        ok = ok and np.array_equal(na, nc)
        if ok:
            idx = np.arange(va["alnOff"][-1]) + np.repeat(vc["alnOff"][:-1][read] - va["alnOff"][:-1], na)
            ok = np.array_equal(va["alignment"], vc["alignment"][idx])
    return bool(ok)


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


def one_chunk(shape, genome, reads, pairs, wb, rows, rotate):
    kind, mode, task, m, _ = SHAPES[shape]
    rb = read_batch(shape, reads, genome, "distance")
    try:
        stats, run_ms = timed(rb.run)
        _, view_ms = timed(lambda: rb.results_flat(copy=False))
        if rows is not None:
            rows["d"].append({"run_ms": run_ms, "view_ms": view_ms, "device_run_ms": stats["run_ms"]})
        tup = tuples_of(rb, m)
        wb.set_units(reads, tup[0], tup[1], tup[2], unit_strand=tup[3])
        order = (["a", "b", "b2", "w"] * 2)[rotate % 4:rotate % 4 + 4]
        views = {}
        for leg in order:
            if leg == "a":
                r, v = leg_a(pairs["a"], rb, m)
            elif leg == "w":
                r, v = leg_w(pairs["w"], wb, tup)
            else:
                r, v = leg_b(pairs["b"], genome, reads, rb, m)
            if rows is not None:
                rows[leg].append(r)
            # (every leg's view is copied behind its clock: the resident batches run again)
            views[leg] = {f: None if x is None else np.array(x) for f, x in v.items()}
    finally:
        rb.close()
    for leg in ("b", "b2", "w"):
        assert same_views(views["a"], views[leg]), (shape, rotate, leg)
    rc, vc = leg_c(shape, reads, genome)
    if mode == "HW":
        assert first_hits_equal(views["a"], tup, vc, task == "path"), (shape, rotate, "c")
    if rows is not None:
        rows["c"].append(rc)
    return len(tup[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=262144)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pairs_reads.json"))
    a = ap.parse_args()
    genome = synth.random_dna(12345, a.genome)
    res = {"metric": "bench_pairs_reads", "pairs": a.pairs, "chunks": a.chunks, "genome": a.genome, "shapes": {}}
    for shape in a.shapes.split(","):
        kind, mode, task, m, k = SHAPES[shape]
        rows = {"a": [], "b": [], "b2": [], "w": [], "c": [], "d": []}
        reads = chunk_of(shape, genome, a.pairs, 99)
        n = len(reads)
        z = np.zeros(1, dtype=np.int32)
        wb = edlib_amd.WindowBatch(reads[:1], genome, z, z, z + m, mode="HW", unit_strand=np.zeros(1, dtype=np.uint8))
        pairs = {leg: edlib_amd.PairBatch([], [], mode=mode, task=task) for leg in ("a", "b", "w")}
        try:
            one_chunk(shape, genome, reads, pairs, wb, None, 0)            # warm-up: code objects, the batches' buffers
            mapped = []
            for c in range(a.chunks):
                mapped.append(one_chunk(shape, genome, chunk_of(shape, genome, a.pairs, 100 + c), pairs, wb, rows, c))
        finally:
            for pb in pairs.values():
                pb.close()
            wb.close()
        s = {leg: summary(rs) for leg, rs in rows.items() if leg not in ("c", "d")}
        for leg in ("c", "d"):
            s[leg] = {f: float(np.median([r[f] for r in rows[leg]])) for f in ("run_ms", "view_ms", "device_run_ms")}
        paths_in_read_batch = s["c"]["run_ms"] + s["c"]["view_ms"] - s["d"]["run_ms"] - s["d"]["view_ms"]
        b_set = 0.5 * (s["b"]["set_ms"] + s["b2"]["set_ms"])
        set_noise = abs(s["b"]["set_ms"] - s["b2"]["set_ms"])
        b_run = 0.5 * (s["b"]["device_run_ms"] + s["b2"]["device_run_ms"])
        run_noise = abs(s["b"]["device_run_ms"] - s["b2"]["device_run_ms"])
        res["shapes"][shape] = {
            "reads": n, "read": m, "k": k, "source": kind, "pairs_median": float(np.median(mapped)),
            "a": s["a"], "b": s["b"], "b2": s["b2"], "w": s["w"], "c": s["c"], "d": s["d"], "views_equal": True,
            "first_hits_equal_c": mode == "HW",
            "word_steps_equal": s["a"]["word_steps"] == s["b"]["word_steps"] == s["b2"]["word_steps"] == s["w"]["word_steps"],
            "set_b_over_a": b_set / max(s["a"]["set_ms"], 1e-9),
            "set_b_legs_differ_ms": set_noise,
            # the bar: (a)'s set below (b)'s by more than the two (b) legs differ
            "a_set_below_b_set": s["a"]["set_ms"] < b_set - set_noise,
            "a_set_minus_w_set_ms": s["a"]["set_ms"] - s["w"]["set_ms"],
            "a_set_within_noise_of_w": abs(s["a"]["set_ms"] - s["w"]["set_ms"]) <= set_noise,
            # (a)'s materialise_ms is first_hit_windows alone; (b)'s holds it, too
            "materialise_ms_saved": 0.5 * (s["b"]["materialise_ms"] + s["b2"]["materialise_ms"]) - s["a"]["materialise_ms"],
            "device_run_b_legs_differ_ms": run_noise,
            "device_run_a_minus_b_ms": s["a"]["device_run_ms"] - b_run,
            "a_run_within_noise": abs(s["a"]["device_run_ms"] - b_run) <= run_noise,
            "chunk_b_over_a": 0.5 * (s["b"]["chunk_ms"] + s["b2"]["chunk_ms"]) / max(s["a"]["chunk_ms"], 1e-9),
            "c_beyond_d_ms": paths_in_read_batch,
            "c_beyond_d_over_a_chunk": paths_in_read_batch / max(s["a"]["chunk_ms"], 1e-9)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
