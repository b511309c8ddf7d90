#!/usr/bin/env python3
"""What searching both strands costs: config 2's batch of bench.py (N x 150 bp HW reads against the 5 Mb
target, k = -1, distances) with every second read reverse-complemented, as
  (a) a both-strand batch of the N reads (edlibAmdBatchCreateSharedBothStrands),
  (b) the way without it: a shared-target batch over the 2N host-made sequences, the better strand picked on the host,
  (c) config 2 itself: the N forward reads on one strand, the yardstick.
Three alternating repetitions after one warm-up run each, medians; the results of the legs are compared.  One JSON line,
to stdout and to --out (default profiles/bench_strands.json).  --b-div D runs leg (b) on the first N / D reads (stated in the
line) when a full step of it does not fit the time there is."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import edlib_amd                      # noqa: E402
from edlib_amd import synth           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--target", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--b-div", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_strands.json"))
    args = ap.parse_args()
    n = args.reads
    target = synth.random_dna(12345, args.target)
    fwd = np.ascontiguousarray(synth.illumina_reads(target, n, m=150, seed=12346)["reads"])
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    mixed = fwd.copy()
    mixed[1::2] = comp[fwd[1::2, ::-1]]                             # every second read comes from the reverse strand
    nb = n // args.b_div
    doubled = np.empty((2 * nb, 150), dtype=np.uint8)
    doubled[0::2] = mixed[:nb]
    doubled[1::2] = comp[mixed[:nb, ::-1]]
    legs = {"a": edlib_amd.BothStrandsBatch(mixed, target, mode="HW", task="distance", k=-1),
            "b": edlib_amd.SharedBatch(doubled, target, mode="HW", task="distance", k=-1),
            "c": edlib_amd.SharedBatch(fwd, target, mode="HW", task="distance", k=-1)}
    run_ms = {x: [] for x in legs}
    wall_ms = {x: [] for x in legs}
    view_ms = {x: [] for x in legs}
    steps, res = {}, {}
    try:
        for x in legs:
            legs[x].run()
        for _ in range(args.reps):
            for x in ("a", "b", "c"):
                t0 = time.perf_counter()
                st = legs[x].run()
                wall_ms[x].append((time.perf_counter() - t0) * 1e3)
                t1 = time.perf_counter()
                res[x] = legs[x].results_flat(copy=False)["editDistance"].copy()
                view_ms[x].append((time.perf_counter() - t1) * 1e3)
                run_ms[x].append(st["run_ms"])
                steps[x] = st["word_steps"]
        strand, both = legs["a"].strands()
    finally:
        for b in legs.values():
            b.close()
    # (b) resolved on the host by the same rule: the forward strand wins a tie
    dp, dm = res["b"][0::2], res["b"][1::2]
    b_strand = (dm < dp).astype(np.uint8)
    b_best = np.where(b_strand == 1, dm, dp)
    ab = int(np.sum(res["a"][:nb] != b_best)) + int(np.sum(strand[:nb] != b_strand)) + int(np.sum(both[:nb] != (dp == dm)))
    # (c) saw the original strand of every read: that is the strand (a) reports wherever the other one is not as good
    same = (strand == (np.arange(n) % 2)) | (both == 1)
    ac = int(np.sum(res["a"][same] != res["c"][same])) + int(np.sum(res["a"] > res["c"]))
    med = {x: statistics.median(run_ms[x]) for x in legs}
    line = {"tool": "bench_strands", "reads": n, "target": args.target, "reps": args.reps, "b_reads": nb, "b_div": args.b_div,
            "run_ms": {x: round(med[x], 3) for x in legs},
            "wall_ms": {x: round(statistics.median(wall_ms[x]), 3) for x in legs},
            "view_ms": {x: round(statistics.median(view_ms[x]), 3) for x in legs},
            "word_steps": steps,
            "a_over_c_run_ms": round(med["a"] / med["c"], 3), "a_over_c_word_steps": round(steps["a"] / steps["c"], 3),
            "b_over_a_run_ms_scaled": round(med["b"] * args.b_div / med["a"], 3),
            "b_over_a_word_steps_scaled": round(steps["b"] * args.b_div / steps["a"], 3),
            "strands": {"forward": int(np.sum(strand == 0)), "reverse": int(np.sum(strand == 1)), "both": int(both.sum())},
            "mismatches_a_vs_b": ab, "mismatches_a_vs_c": ac}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0 if ab == 0 and ac == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
