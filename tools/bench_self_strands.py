"""Both-strand self batches (every unordered pair once, in its better orientation) beside the both-strand cross batch given
the same pool twice and beside the one-strand self batch, on one device; medians of resident runs, the three legs
alternating in one process.

The de-duplication shape with unknown orientation: 200,000 x 32 bp in 2,000 families of 100, every second sequence
reverse-complemented, NW, k = 2, hit lists -- SelfBatch(hits=True, strands="both") beside
CrossBatch(seqs, seqs, hits=True, strands="both") and SelfBatch(hits=True).  By the counters the both-strand self scan is
(n - 1) / 2n of the both-strand cross scan (required of word_steps: <= 0.60) and twice the one-strand self scan; the
measured times are recorded, not gated.  Sampled hits are checked against the reference on both orientations.  Prints
one JSON line and writes profiles/bench_self_strands.json.

    python tools/bench_self_strands.py [--families 2000] [--runs 5] [--check 2000]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import edlib_amd  # noqa: E402
from bench_cross import families  # noqa: E402
from bench_self import alternate, timed  # noqa: E402


def reference(seqs, i, j, k):
    """(distance, strand byte) of the pairs (i, j), i < j, by the reference on both orientations"""
    from oracle import oracle as O

    def pack(s):
        off = np.zeros(len(s) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in s])
        return np.frombuffer(b"".join(s) + b"\0", dtype=np.uint8), off
    tp, to = pack([bytes(seqs[int(b)]) for b in j])
    d = []
    for q in ([bytes(seqs[int(a)]) for a in i], [edlib_amd.reverse_complement(bytes(seqs[int(a)])) for a in i]):
        qp, qo = pack(q)
        d.append(np.asarray(O.pool_align(qp, qo, tp, to, False, "NW", "distance", k)["editDistance"]))
    return edlib_amd.self_strands_model(d[0], d[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=2000, help="families of 100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=2000)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    seqs = [bytes(s) for s in families(rng, a.families, 100)]
    seqs = [edlib_amd.reverse_complement(s) if x & 1 else s for x, s in enumerate(seqs)]
    n = len(seqs)
    both = edlib_amd.SelfBatch(seqs, k=2, hits=True, strands="both")
    cross = edlib_amd.CrossBatch(seqs, seqs, mode="NW", k=2, hits=True, strands="both")
    one = edlib_amd.SelfBatch(seqs, k=2, hits=True)
    leg = alternate({"self_both": both, "cross_both": cross, "self_forward": one}, a.runs)
    h, leg["self_both"]["view_hits_ms"] = timed(lambda: both.hits(copy=False))
    s, leg["self_both"]["view_strands_ms"] = timed(lambda: both.strands(copy=False))
    _, leg["self_both"]["view_nearest_ms"] = timed(lambda: both.nearest(copy=False))
    ch, leg["cross_both"]["view_hits_ms"] = timed(lambda: cross.hits(copy=False))
    leg["self_both"]["numHits"] = int(len(h["partner"]))
    leg["self_both"]["reverse_hits"] = int(np.count_nonzero(s["hitStrand"] & 1))
    leg["cross_both"]["numHits"] = int(len(ch["query"]))
    leg["self_forward"]["numHits"] = int(len(one.hits(copy=False)["partner"]))
    row = np.repeat(np.arange(n), np.diff(h["rowOffsets"]))
    pick = rng.choice(len(row), size=min(a.check, len(row)), replace=False)
    we, ws = reference(seqs, row[pick], h["partner"][pick], 2)
    leg["sample_mismatches"] = int(np.sum(we != h["editDistance"][pick]) + np.sum(ws != s["hitStrand"][pick]))
    leg["shape"] = [n, 32]
    leg["k"] = 2
    for f in ("scan", "run"):
        leg[f + "_ratio_to_cross_both"] = leg["self_both"][f + "_ms"] / max(leg["cross_both"][f + "_ms"], 1e-9)
        leg[f + "_ratio_to_self_forward"] = leg["self_both"][f + "_ms"] / max(leg["self_forward"][f + "_ms"], 1e-9)
    leg["word_steps_ratio"] = leg["self_both"]["word_steps"] / max(leg["cross_both"]["word_steps"], 1)
    leg["word_steps_ratio_required"] = 0.60
    res = {"metric": "bench_self_strands", "hits_200k_32_both": leg}
    for b in (both, cross, one):
        b.close()

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_self_strands.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
