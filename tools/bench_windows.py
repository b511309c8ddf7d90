#!/usr/bin/env python3
"""Window batches against pair batches on the verification step of a seed-and-extend mapper: n reads of 150 bases, each
HW against a 400-base window of the 5 Mb target around its origin (the first shape of tools/bench_short_pairs.py).
Three legs, alternating, the median of 5 resident runs each, in one process:
 (a) WindowBatch over (read, start, 400): Create wall time (upload + pack), run_ms, scan_ms, the UNITS view;
 (b) PairBatch over the windows materialised with numpy: the time to materialise them, Create wall time, run_ms,
     results_flat(copy=False);
 (c) n / 4 reads x 4 candidate windows (one true, three random) as a window batch: run_ms and the BEST-only view.
A strided sample of 256 units of every leg is checked against the oracle.  One JSON line, also written to
profiles/bench_windows.json."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import edlib_amd
from edlib_amd import synth
from oracle import oracle as O

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
RUNS, M, W = 5, 150, 400
T = synth.random_dna(12345, 5_000_000)
R = synth.illumina_reads(T, n, m=M)
reads, pos = R["reads"], np.asarray(R["start"], dtype=np.int64)
start = np.clip(pos - 125, 0, len(T) - W)


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def sample_ok(ed, q, us):
    """ed of a strided sample of 256 units against the oracle on the sliced bytes."""
    sel = np.arange(0, len(us), max(1, len(us) // 256))
    wins = np.ascontiguousarray(T[us[sel][:, None] + np.arange(W)[None, :]])
    qs = np.ascontiguousarray(reads[q[sel]])
    ref = O.pool_align(qs.reshape(-1), np.arange(len(sel) + 1, dtype=np.int64) * M, wins.reshape(-1),
                       np.arange(len(sel) + 1, dtype=np.int64) * W, False, "HW", "distance", -1)
    return bool(np.array_equal(np.asarray(ed)[sel], ref["editDistance"]))


med = lambda x: round(float(np.median(x)), 3)
ident = np.arange(n, dtype=np.int32)
length = np.full(n, W, dtype=np.int32)

# (a)
a, a_create = ms(lambda: edlib_amd.WindowBatch(reads, T, ident, start, length, mode="HW"))
# (b)
win, b_mat = ms(lambda: np.ascontiguousarray(T[start[:, None] + np.arange(W)[None, :]]))
b, b_create = ms(lambda: edlib_amd.PairBatch(reads, win, mode="HW", task="distance"))
# (c)
nc = n // 4
rng = np.random.default_rng(1)
cs = rng.integers(0, len(T) - W + 1, size=(nc, 4))
slot = rng.integers(0, 4, size=nc)
cs[np.arange(nc), slot] = start[:nc]
cs = cs.reshape(-1)
cq = np.repeat(np.arange(nc, dtype=np.int32), 4)
c, c_create = ms(lambda: edlib_amd.WindowBatch(reads[:nc], T, cq, cs, np.full(4 * nc, W, dtype=np.int32), mode="HW"))

for x in (a, b, c):                                     # warm-up: the pinned blocks of the sessions
    x.run()
a.units(copy=False); b.results_flat(copy=False); c.best(copy=False)
t = {k: [] for k in ("a_run", "a_scan", "a_view", "b_run", "b_scan", "b_view", "c_run", "c_scan", "c_view")}
for _ in range(RUNS):
    st = a.run(); t["a_run"].append(st["run_ms"]); t["a_scan"].append(st["scan_ms"])
    au, v = ms(lambda: a.units(copy=False)); t["a_view"].append(v)
    a_stats = st
    st = b.run(); t["b_run"].append(st["run_ms"]); t["b_scan"].append(st["scan_ms"])
    bf, v = ms(lambda: b.results_flat(copy=False)); t["b_view"].append(v)
    b_stats = st
    st = c.run(); t["c_run"].append(st["run_ms"]); t["c_scan"].append(st["scan_ms"])
    cb, v = ms(lambda: c.best(copy=False)); t["c_view"].append(v)
    c_stats = st
cu = c.units()
true_unit = 4 * np.arange(nc) + slot
ed4 = cu["editDistance"].reshape(nc, 4)
others = np.where(np.arange(4)[None, :] == slot[:, None], np.iinfo(np.int32).max, ed4).min(axis=1)
clear = ed4[np.arange(nc), slot] < others
out = {
    "units": n, "read": M, "window": W, "runs": RUNS,
    "a_windows": {"create_ms": round(a_create, 2), "run_ms": med(t["a_run"]), "scan_ms": med(t["a_scan"]),
                  "units_view_ms": med(t["a_view"]), "word_steps": a_stats["word_steps"], "path": a_stats["path"],
                  "word_steps_per_s": round(a_stats["word_steps"] / (np.median(t["a_scan"]) * 1e-3), 0),
                  "sample_ok": sample_ok(au["editDistance"], ident, start)},
    "b_pairs": {"materialise_ms": round(b_mat, 2), "create_ms": round(b_create, 2), "run_ms": med(t["b_run"]),
                "scan_ms": med(t["b_scan"]), "results_view_ms": med(t["b_view"]), "path": b_stats["path"],
                "sample_ok": sample_ok(bf["editDistance"], ident, start),
                "equals_a": bool(np.array_equal(bf["editDistance"], au["editDistance"]))},
    "c_four_candidates": {"reads": nc, "units": 4 * nc, "create_ms": round(c_create, 2), "run_ms": med(t["c_run"]),
                          "scan_ms": med(t["c_scan"]), "best_view_ms": med(t["c_view"]),
                          "sample_ok": sample_ok(cu["editDistance"], cq, cs),
                          "best_is_true_locus": bool(np.array_equal(cb["bestUnit"][clear], true_unit[clear]))},
}
out["a_run_over_b_run"] = round(out["a_windows"]["run_ms"] / out["b_pairs"]["run_ms"], 3)
for x in (a, b, c):
    x.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "bench_windows.json"), "w") as f:
    f.write(line + "\n")
