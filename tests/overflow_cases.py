"""Planted batches and the CPU model for the exact pass of HW read groups (Batch::runGroupExact): a slot with
more than 16 end locations gets its complete list either GATHERED from the segment records of the scan that answered it
(every segment that holds the best score kept all of its hits) or from a RESCAN (some segment held more hits than its cap).

The model restates merge_segments_kernel + gather_segments_kernel in numpy (tests/test_overflow_model.py holds it against a
plain sort), and expected_exact_pass() derives, from the REFERENCE's end locations and the segmentation the engine printed,
how many slots of a group go which way."""
import numpy as np

from edlib_amd import synth
from seed_cases import _ACGT, _reads
from seed_model import seed_threshold

CAP_FINAL = 16          # positions a slot keeps (kPosCap of the merge)
CAP_PASS1 = 8           # positions per (lane, segment) of pass 1 and of the levels below the last
CAP_LAST = 16           # ... of the last level (Batch::kLastLevelCap)


# ---------------------------------------------------------------------------------------------------------------- the model

def segment_records(cols, scores, seg_len, S, cap):
    """what a scan leaves per segment for one lane whose columns `cols` (ascending) score `scores` (only columns at or below
    the lane's threshold are given): best score, number of columns attaining it (counted past the cap), the first `cap`"""
    best = np.full(S, 0x7fffffff, dtype=np.int64)
    cnt = np.zeros(S, dtype=np.int64)
    pos = np.full((S, cap), -1, dtype=np.int64)
    for c, s in zip(cols, scores):
        g = int(c) // seg_len
        if s < best[g]:
            best[g], cnt[g] = s, 0
        if s == best[g]:
            if cnt[g] < cap:
                pos[g, cnt[g]] = c
            cnt[g] += 1
    return best, cnt, pos


def merge_gather(best, cnt, pos, cap, cap_final=CAP_FINAL):
    """merge_segments_kernel: (best or -1, total, the first cap_final positions, reason) with reason 0 = the list fits,
    1 = a contributing segment overflowed its cap, 2 = only the final list overflowed; and gather_segments_kernel's list
    (None unless reason 2)"""
    live = cnt > 0
    if not live.any():
        return -1, 0, [], 0, None
    b = int(best[live].min())
    contrib = np.flatnonzero(live & (best == b))
    total = int(cnt[contrib].sum())
    listed = [int(pos[g, i]) for g in contrib for i in range(min(int(cnt[g]), cap))]
    reason = 1 if (cnt[contrib] > cap).any() else (2 if total > cap_final else 0)
    return b, total, listed[:cap_final], reason, (listed if reason == 2 else None)


def reason_of(ends, seg_len, cap, cap_final=CAP_FINAL):
    """the same decision from a slot's complete ascending end locations alone (what the reference gives)"""
    ends = np.asarray(ends, dtype=np.int64)
    if len(ends) <= cap_final and (len(ends) == 0 or np.bincount(ends // seg_len).max() <= cap):
        return 0
    return 1 if np.bincount(ends // seg_len).max() > cap else 2


def expected_exact_pass(ref, idx, k_first, seeded, seg_pass1, seg_last, seg_levels=None):
    """(gathered, rescanned) for the group of the reads `idx`: ref = the reference's flat results, k_first = the threshold of
    pass 1, seeded = pass 1 was the seed filter, seg_pass1 / seg_last = columns per segment of the banded pass 1 / of the
    last level, seg_levels = {threshold: columns per segment} of the ladder's levels in between (they keep 8 positions per
    segment and their records do not outlive them: every overflow there is rescanned).  The seed filter keeps no segment records: a read it answers is rescanned when it has
    more than 16 end locations (also when the filter handed it back to the banded scan -- the batches here hold no handed-back
    read with 9 .. 16 end locations in one segment, which that scan would flag as well)."""
    gathered = rescanned = 0
    lo = ref["locOff"]
    for u in idx:
        d = int(ref["editDistance"][u])
        ends = ref["ends"][lo[u]:lo[u + 1]]
        if d < 0:
            continue
        mid = sorted(t for t in (seg_levels or {}) if t >= d)
        if d > k_first and mid:
            r = 1 if reason_of(ends, seg_levels[mid[0]], CAP_PASS1) else 0
        elif d > k_first:
            r = reason_of(ends, seg_last, CAP_LAST)
        elif seeded:
            r = 1 if len(ends) > CAP_FINAL else 0
        else:
            r = reason_of(ends, seg_pass1, CAP_PASS1)
        gathered += r == 2
        rescanned += r == 1
    return gathered, rescanned


# -------------------------------------------------------------------------------------------------------------- the batches

def _substitute(rng, w, n):
    """n substitutions at distinct positions away from both ends (what follows a copy in the target must not matter)"""
    w = w.copy()
    for p in 8 + rng.choice(len(w) - 16, n, replace=False):
        w[p] = _ACGT[(np.searchsorted(_ACGT, w[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return np.ascontiguousarray(w)


def planted(T=256_000, n_fill=4_400, seed=7100, five=False, task="distance"):
    """Reads of five words (129 .. 160 bases; the planted ones 150) against T columns, k = -1.  Three random blocks copied 17, 40 and 64 times, 1,600 columns apart (far
    more than a read apart, 17 .. 64 copies never crowd a segment of >= 4,096 columns past eight); two tandem runs of 120
    units ACGTG (a read of 30 units fits at 91 shifts of a run: far more than 16 end locations five columns apart inside one
    segment, and both runs in one list).  Planted reads: every block and 30 units, each as it is and with 3 substitutions
    (answered by pass 1) and with 12 substitutions (answered by the last level).  five: N's in the target (five symbols:
    the group keeps the banded first pass).  claims[i] = number of copies of read i's block, or 0 for a tandem read, or None"""
    rng = np.random.default_rng(seed)
    target = synth.random_dna(seed + 1, T).copy()
    lo = 8_192
    blocks, at = [], lo
    for copies in (17, 40, 64):
        b = synth.random_dna(seed + 10 + copies, 150)
        for j in range(copies):
            target[at:at + 150] = b
            at += 1_600
        blocks.append((b, copies))
    runs = (at + 2_000, at + 40_000)
    unit = np.frombuffer(b"ACGTG", dtype=np.uint8)
    for r in runs:
        target[r:r + 600] = np.tile(unit, 120)
    hi = runs[1] + 600
    assert hi + 1_000 < T
    if five:
        free = np.concatenate([np.arange(1_000, lo - 1_000), np.arange(hi + 1_000, T - 1_000)])
        target[rng.choice(free, 300, replace=False)] = ord("N")
    reads, claims = [], []
    for b, copies in blocks:
        for subs in (0, 3, 12, 12):
            reads.append(_substitute(rng, b, subs) if subs else np.ascontiguousarray(b))
            claims.append(copies)
    for subs in (0, 3, 12, 12):
        w = np.tile(unit, 30)
        if subs:                                                   # evenly spread, away from both ends
            w = w.copy()
            for p in np.linspace(10, 140, subs).astype(int):
                w[p] = _ACGT[(np.searchsorted(_ACGT, w[p]) + 1 + int(rng.integers(0, 3))) % 4]
        reads.append(np.ascontiguousarray(w))
        claims.append(0)
    kf = seed_threshold(131, T)
    fill = _reads(target, n_fill, seed + 2, kf, mlo=138, mhi=151, avoid=(lo - 200, hi + 200))
    order = rng.permutation(len(reads) + len(fill))
    allr, allc = reads + fill, claims + [None] * len(fill)
    return {"reads": [allr[i] for i in order], "claims": [allc[i] for i in order], "target": target, "k": -1, "task": task}


def launches(n=45_056, T=131_072, unrelated=0.095, crowded=False, seed=7300):
    """n reads of five words (129 .. 160 bases) against a uniform random target, k = -1: `unrelated` of them random (the leftovers of the
    last level), the others within the seed threshold.  crowded: a block copied 40 times 160 columns apart (a segment of
    >= 4,096 columns holds at least 20 of them) and three reads of it with 12 substitutions, one in every piece of the seed
    filter (no seed hits, so the filter does not hand them back): more than 16 end locations in one segment, the exact pass
    scans them again"""
    rng = np.random.default_rng(seed)
    target = synth.random_dna(seed + 1, T).copy()
    kf = seed_threshold(131, T)
    avoid = None
    if crowded:
        b = synth.random_dna(seed + 3, 150)
        for j in range(40):
            target[60_000 + 160 * j:60_000 + 160 * j + 150] = b
        avoid = (59_000, 60_000 + 160 * 40 + 1_000)
    reads = _reads(target, n - (3 if crowded else 0), seed + 2, kf, mlo=138, mhi=151, unrelated=unrelated, above=0.0,
                   with_n=0.0, avoid=avoid)
    if crowded:
        K = seed_threshold(min(len(r) for r in reads), T)           # the engine's threshold: K + 1 pieces of a 150-base read
        assert kf <= K < 12
        L, r = 150 // (K + 1), 150 % (K + 1)
        for _ in range(3):
            w = b.copy()
            at = [i * L + min(i, r) + int(rng.integers(2, L - 2)) for i in range(K + 1)]
            at += [int(x) for x in rng.choice(sorted(set(range(150)) - set(at)), 12 - len(at), replace=False)]
            for p in at:
                w[p] = _ACGT[(np.searchsorted(_ACGT, w[p]) + 1 + int(rng.integers(0, 3))) % 4]
            reads.append(np.ascontiguousarray(w))
    return {"reads": reads, "target": target, "k": -1, "task": "distance"}


def batch(name):
    kind, _, arg = name.partition(":")
    if kind == "planted":
        return planted(task=arg or "distance")
    if kind == "planted5":
        return planted(five=True, task=arg or "distance", seed=7200)
    if kind == "launches":
        return {"few": lambda: launches(), "crowded": lambda: launches(crowded=True, seed=7400),
                "open": lambda: launches(unrelated=0.13, seed=7500)}[arg]()
    raise KeyError(name)
