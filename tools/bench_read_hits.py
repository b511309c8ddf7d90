"""Hit-list read batches (SharedBatch(..., hits=True)) on one device, each beside a plain SharedBatch DISTANCE run at the
same k on the same inputs in the same process: median resident run ms, scan ms, word_steps, and for the hit list its
numHits, first-run ms (a first Run past the list's capacity grows it) and the hits-view ms.

  * config 2's shape (bench.py: 150 bp reads, 1 % substitutions, 0.05 % indels, 5 % unrelated, against one 5 Mb uniform
    ACGT target) at k = 3 and at k = k_f, the seed filter's threshold for that shape;
  * 96 x 24 bp primers against the 5 Mb target at k = 2;
  * 16,384 of those reads at k = k_f + 3: above the seed threshold, so the hit list takes the banded HITS scan of a
    five-word group (the instances that spill under the eight-wave bound) while the plain batch takes the
    seed pass at k_f and one level above it.

No ratio is fixed in advance: the plain run at the same fixed k is the yardstick, the expectation to confirm or refute is
"about the same".  Prints one JSON line and writes it to profiles/bench_read_hits.json.

    python tools/bench_read_hits.py [--reads 1000000] [--runs 5] [--out profiles/bench_read_hits.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import edlib_amd  # noqa: E402
from edlib_amd import synth  # noqa: E402

TARGET_LEN, READ_LEN = 5_000_000, 150


def seed_threshold(m_min, T, q=12, kmax=16):
    """Batch::seedThreshold's k_f"""
    for k in range(kmax, -1, -1):
        L = m_min // (k + 1)
        if L >= q and (k + 1) * T * 8 <= 4 ** L:
            return k
    return -1


def time_batch(reads, target, k, runs, hits):
    b = edlib_amd.SharedBatch(reads, target, mode="HW", task="distance", k=k, hits=hits)
    try:
        st = b.run()                                        # warm-up
        out = {"first_run_ms": st["run_ms"]}
        ms, scan = [], []
        for _ in range(runs):
            t = time.perf_counter()
            st = b.run()
            ms.append((time.perf_counter() - t) * 1e3)
            scan.append(st["scan_ms"])
        out.update(run_ms=float(np.median(ms)), scan_ms=float(np.median(scan)), word_steps=st["word_steps"],
                   scan_launches=st["scan_launches"])
        t = time.perf_counter()
        if hits:
            h = b.hits(copy=False)
            out.update(view_ms=(time.perf_counter() - t) * 1e3, numHits=int(h["numHits"]),
                       reads_with_hits=int(np.count_nonzero(np.diff(h["unitOffsets"]))))
        else:
            r = b.results_flat(copy=False)
            out.update(view_ms=(time.perf_counter() - t) * 1e3, reads_within_k=int(np.count_nonzero(r["editDistance"] >= 0)))
        return out
    finally:
        b.close()


def side_by_side(name, reads, target, k, runs):
    plain = time_batch(reads, target, k, runs, False)
    hits = time_batch(reads, target, k, runs, True)
    assert hits["reads_with_hits"] == plain["reads_within_k"], (name, hits, plain)
    return {"name": name, "reads": len(reads), "read_len": int(len(reads[0])), "target_len": len(target), "k": k,
            "hits": hits, "plain": plain, "run_ms_ratio": hits["run_ms"] / plain["run_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_read_hits.json"))
    a = ap.parse_args()
    assert edlib_amd.device_count() >= 1, edlib_amd.last_error()
    target = synth.random_dna(12345, TARGET_LEN)
    kf = seed_threshold(READ_LEN, TARGET_LEN)
    rng = np.random.default_rng(12347)
    primers = np.ascontiguousarray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (96, 24))])
    target = target.copy()
    for i in range(0, 96, 2):                               # half of the primers occur, ten times each
        for at in rng.integers(0, TARGET_LEN - 24, 10):
            target[at:at + 24] = primers[i]
    reads = np.ascontiguousarray(synth.illumina_reads(target, a.reads, m=READ_LEN, seed=12346)["reads"])
    cases = [side_by_side("config2_k3", reads, target, 3, a.runs),
             side_by_side("config2_kf", reads, target, kf, a.runs),
             side_by_side("primers_k2", primers, target, 2, a.runs),
             side_by_side("banded_kf_plus_3", reads[:16_384], target, kf + 3, a.runs)]
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    line = json.dumps({"bench": "read_hits", "date": time.strftime("%Y-%m-%d"), "commit": commit, "k_f": kf, "runs": a.runs,
                       "cases": cases})
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
