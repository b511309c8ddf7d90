"""Both-strand read batches (edlibAmdBatchCreateSharedBothStrands): the complement table, rc(), the rule that
picks one strand's result, and the seeded batches of tests/test_strand_model.py (CPU: every batch satisfies what its GPU
test assumes) and tests/test_gpu_strands.py (GPU).  numpy only; inputs come from tests/seed_cases.py, expected results from
the reference run over every read AND its reverse complement (2n alignments) pushed through resolve_flat().

The contract, with d+ / d- the edit distances of q and rc(q) (-1: nothing within k):
    d+ >= 0 and (d- < 0 or d+ <= d-)   ->  the forward result, strand 0, bothStrands = (d- == d+)
    otherwise, d- >= 0                 ->  the result of rc(q), strand 1, bothStrands 0
    d+ == d- == -1                     ->  the forward result (distance -1), strand 0, bothStrands 0
"""
import numpy as np

import seed_model as SM
from seed_cases import M_MIN, _mutate, _reads, fit_lengths

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

_PAIRS = [("A", "T"), ("C", "G"), ("R", "Y"), ("K", "M"), ("B", "V"), ("D", "H")]


def _table():
    c = np.arange(256, dtype=np.uint8)
    for a, b in _PAIRS:
        for x, y in ((a, b), (b, a)):
            c[ord(x)] = ord(y)
            c[ord(x.lower())] = ord(y.lower())
    c[ord("U")], c[ord("u")] = ord("A"), ord("a")
    return c


COMP = _table()
CODES = b"ACGTURYKMBDHVSWNacgturykmbdhvswn"


def rc(q):
    """the reverse complement of a uint8 array (or bytes): rc(q)[j] = COMP[q[m - 1 - j]]"""
    a = np.frombuffer(q, dtype=np.uint8) if isinstance(q, (bytes, bytearray)) else np.asarray(q, dtype=np.uint8)
    return np.ascontiguousarray(COMP[a[::-1]])


def interleave(reads):
    """[q0, rc(q0), q1, rc(q1), ...]"""
    out = []
    for r in reads:
        r = np.ascontiguousarray(r, dtype=np.uint8)
        out += [r, rc(r)]
    return out


def resolve(rp, rm):
    """(reported result, strand, bothStrands) of one read from the two reference results (dicts with editDistance)"""
    dp, dm = rp["editDistance"], rm["editDistance"]
    if dp >= 0 and (dm < 0 or dp <= dm):
        return rp, 0, int(dm == dp)
    if dm >= 0:
        return rm, 1, 0
    return rp, 0, 0


def strands_of(d2):
    """(strand, bothStrands) as uint8 arrays from the 2n distances [d+0, d-0, d+1, d-1, ...]: the table as numpy"""
    dp, dm = np.asarray(d2[0::2]), np.asarray(d2[1::2])
    fwd = (dp >= 0) & ((dm < 0) | (dp <= dm))
    strand = (~fwd & (dm >= 0)).astype(np.uint8)
    both = (fwd & (dm == dp)).astype(np.uint8)
    return strand, both


def take_units(flat, idx, task):
    """the units `idx` of a flat result (oracle.pool_align / results_flat layout), as a flat result of len(idx) units"""
    idx = np.asarray(idx, dtype=np.int64)
    out = {f: flat[f][idx] for f in ("status", "editDistance", "numLocations", "alphabetLength")}

    def gather(off, data):
        lens = off[idx + 1] - off[idx]
        new = np.zeros(len(idx) + 1, dtype=np.int64)
        new[1:] = np.cumsum(lens)
        pick = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) and new[-1] else np.zeros(0, dtype=np.int64)
        return new, data[pick.astype(np.int64)]
    out["locOff"], out["ends"] = gather(flat["locOff"], flat["ends"])
    out["starts"] = gather(flat["locOff"], flat["starts"])[1] if task != "distance" else None
    out["alnOff"], out["alignment"] = gather(flat["alnOff"], flat["alignment"])
    return out


def resolve_flat(ref2, task):
    """the flat result of n reads from the reference's flat result over the 2n interleaved sequences, + strand, bothStrands"""
    strand, both = strands_of(ref2["editDistance"])
    idx = 2 * np.arange(len(strand), dtype=np.int64) + strand
    out = take_units(ref2, idx, task)
    out["strand"], out["bothStrands"], out["unit"] = strand, both, idx
    return out


def pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs])
    pool = np.concatenate(seqs) if len(seqs) and off[-1] else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(pool, dtype=np.uint8), off


def reference_both(b, want_cigar=False):
    """the reference over both strands of every read of batch b, resolved: (resolved flat result, the 2n-unit flat result)"""
    from oracle import oracle as O
    pool, off = pack(interleave(b["reads"]))
    ref2 = O.pool_align(pool, off, b["target"], np.array([0, len(b["target"])], dtype=np.int64), True, b["mode"], b["task"],
                        b["k"], eq_pairs=b.get("eq"), want_cigar=want_cigar)
    return resolve_flat(ref2, b["task"]), ref2


# ------------------------------------------------------------------------------------------------------ small cases (CPU)

def table_rows():
    """(name, read, target, mode, k) covering every row of the table, a palindrome and an empty read"""
    t = b"TTGACCATGCAAGTCCTGATCGGATTACAGCATTGCAAGGCTCTAGCGATTTCAGG"
    fwd = t[5:35]
    worse = bytearray(fwd); worse[3] = ord("A") if worse[3] != ord("A") else ord("C")
    pal = b"ACGTTGCATGCAACGT"
    assert bytes(rc(pal)) == pal
    return [
        ("forward only within k", fwd, t, "HW", 2),
        ("reverse only within k", bytes(rc(fwd)), t, "HW", 2),
        ("forward better, both within k", fwd, t, "HW", -1),
        ("reverse better, both within k", bytes(rc(bytes(worse))), t, "HW", -1),
        ("neither within k", b"GGGGGGGGGGGGGGGGGGGGGG", b"ATATATATATATATATATATATATAT", "HW", 1),
        ("palindrome", pal, t[:20] + pal + t[20:], "HW", -1),
        ("tie of two different strands", b"AC", b"ACGT", "HW", -1),
        ("empty read", b"", t, "HW", -1),
        ("NW", fwd, bytes(rc(fwd)), "NW", -1),
        ("SHW reverse", bytes(rc(t[:25])), t, "SHW", -1),
    ]


# ------------------------------------------------------------------------------------------- the GPU tests' batches

def _flip(reads, every=2, first=1):
    """every second read taken from the reverse strand"""
    return [rc(r) if i % every == first else np.ascontiguousarray(r) for i, r in enumerate(reads)]


def palindrome(rng, m, alphabet=_ACGT):
    half = alphabet[rng.integers(0, len(alphabet), m // 2)]
    p = np.concatenate([half, rc(half)])
    assert np.array_equal(rc(p), p)
    return np.ascontiguousarray(p)


# bytes the complement table leaves alone: the pair route's alphabet (a shared target of more than four symbols, SHW / NW)
PLAIN20 = np.frombuffer(b"EFIJLOPQXZNSW0123456", dtype=np.uint8)
assert np.array_equal(COMP[PLAIN20], PLAIN20) and len(set(PLAIN20.tolist())) == 20


def parity_batches(mode, task, k, seed=0):
    """test 1: the batches of one (mode, task, k): every route of a both-strand batch.  HW: targets of 30,000 .. 60,000
    columns over ACGT and over ACGT + N; SHW / NW: targets about as long as the reads over ACGT, over ACGT + N, and over 20
    symbols that the table leaves alone (400 and 1,200 reads: below and above the 1,024 internal pair units from which a
    single-strand batch of short pairs takes the flat path)."""
    out = []
    kinds = ("acgt", "acgtn") if mode == "HW" else ("acgt", "acgtn", "plain400", "plain1200")
    for ti, kind in enumerate(kinds):
        rng = np.random.default_rng(1000 * seed + 97 * ti + 13 * (k + 2) + {"HW": 0, "SHW": 1, "NW": 2}[mode] * 7 +
                                    {"distance": 0, "locations": 3, "path": 5}[task])
        if kind.startswith("plain"):
            n = int(kind[5:])
            T = 260
            target = PLAIN20[rng.integers(0, 20, T)].copy()
            reads = []
            for i in range(n):
                m = int(rng.integers(20, 257))
                u = rng.random()
                if u < 0.1:
                    r = PLAIN20[rng.integers(0, 20, m)]
                else:
                    s = int(rng.integers(0, T - m + 1))
                    r = target[s:s + m].copy()
                    for _ in range(int(rng.integers(0, 7))):
                        r[int(rng.integers(0, m))] = PLAIN20[rng.integers(0, 20)]
                    if mode == "SHW" and i % 3 == 0:
                        r = target[:m].copy()
                reads.append(np.ascontiguousarray(r))
            reads[0] = np.zeros(0, dtype=np.uint8)
            reads[1] = palindrome(rng, 60, PLAIN20)
            out.append({"name": kind, "reads": _flip(reads), "target": target, "mode": mode, "task": task, "k": k})
            continue
        T = int(rng.integers(30_000, 60_001)) if mode == "HW" else 300
        target = _ACGT[rng.integers(0, 4, T)].copy()
        if kind == "acgtn":
            target[rng.integers(0, T, max(3, T // 400))] = ord("N")
        lengths = [20, 31, 32, 33, 64, 65, 96, 97, 128, 129, 150, 160, 161, 192, 193, 224, 225, 255, 256]
        lengths += [int(x) for x in rng.integers(20, 257, 80)]
        lengths += [300] * 6 + [600] * 4 + [2000] * 3
        reads = []
        for i, m in enumerate(lengths):
            u = rng.random()
            if u < 0.12:                                           # unrelated
                reads.append(np.ascontiguousarray(_ACGT[rng.integers(0, 4, m)]))
                continue
            if m <= T:
                s = 0 if i % 17 == 0 else int(rng.integers(0, T - m + 1))
                w = target[s:s + m]
            else:                                                  # (SHW / NW: reads longer than the target)
                w = np.concatenate([target, _ACGT[rng.integers(0, 4, m - T)]])
            edits = int(rng.integers(0, 4)) if u < 0.6 else int(rng.integers(4, 12)) if u < 0.85 else int(rng.integers(30, 60))
            w = _mutate(rng, w, edits, [int(x) for x in rng.integers(0, m, max(1, edits))])
            w = w[:m] if len(w) >= m else np.concatenate([w, _ACGT[rng.integers(0, 4, m - len(w))]])   # (indels moved it)
            if rng.random() < 0.1:
                w = w.copy()
                w[int(rng.integers(0, len(w)))] = ord("N")
            reads.append(np.ascontiguousarray(w))
        reads.append(np.zeros(0, dtype=np.uint8))                  # an empty read
        for m in (40, 150, 256, 300):
            p = palindrome(rng, m)
            if mode == "HW":
                at = int(rng.integers(0, T - m))
                target[at:at + m] = p                              # found at distance 0 on both strands
            reads.append(p)
        reads.append(np.frombuffer(b"ACGTNNRYKMacgtnryk", dtype=np.uint8).copy())   # codes of both cases
        out.append({"name": kind, "reads": _flip(reads), "target": target, "mode": mode, "task": task, "k": k})
    return out


def _resolves(read, tb, tarr, k, index, present):
    """seed_model.seed_filter (caps on) with the target converted and indexed once: True when the read is found within k"""
    diags = SM.lookup(read, tb, k, SM.Q, index, True, present)
    if diags == "back":
        return False
    ws = SM.windows(diags, len(read), k, len(tb))
    if any(b - a + 1 > SM.MAX_WINDOW for a, b in ws):
        return False
    return any(int(SM.bottom_row(np.asarray(read), tarr[a:b + 1]).min()) <= k for a, b in ws)


def seeded_group(nwd, T=256_000, n=2_230, only_resolving=True, task="distance", index=None):
    """tests 2, 3 and 6: n reads of one word count against T columns at k = -1, odd reads reverse-complemented.
    only_resolving (test 2): no unrelated read, none above k_f, and the reads that seed_model.seed_filter resolves on neither
    strand at k_f are dropped ("dropped" says how many); else seed_cases._reads' defaults (5 % unrelated, 3 % above k_f)."""
    rng = np.random.default_rng(4242 + nwd)
    target = _ACGT[rng.integers(0, 4, T)].copy()
    mlo, mhi = M_MIN[nwd], 32 * nwd
    kf = SM.seed_threshold(mlo, T)
    kw = dict(unrelated=0.0, above=0.0) if only_resolving else {}
    reads = _flip(fit_lengths(_reads(target, n, 99 + nwd, kf, mlo, mhi, **kw), mlo, mhi, nwd))
    b = {"name": "seeded%d" % nwd, "target": target, "mode": "HW", "task": task, "k": -1, "kf": kf, "nwd": nwd, "dropped": 0}
    if only_resolving:
        tb = bytes(target)
        index = SM.build_index(tb, SM.Q) if index is None else index
        present = set(tb)
        keep = [r for r in reads if _resolves(r, tb, target, kf, index, present) or _resolves(rc(r), tb, target, kf, index, present)]
        b["dropped"] = len(reads) - len(keep)
        reads = keep
    b["reads"] = reads
    return b


def banded_group(kind, n=1_500):
    """test 4: groups that take the banded first pass at k = -1 (first threshold 8): three words on a four-symbol target of
    60,000 columns (k_f = 5 < 8), five words on an ACGT + N target"""
    nwd = {"three": 3, "five_n": 5}[kind]
    rng = np.random.default_rng(5150 + nwd)
    T = 60_000
    target = _ACGT[rng.integers(0, 4, T)].copy()
    if kind == "five_n":
        target[rng.integers(0, T, 80)] = ord("N")
    mlo, mhi = M_MIN[nwd], 32 * nwd
    reads = _flip(fit_lengths(_reads(target, n, 77 + nwd, 8, mlo, mhi), mlo, mhi, nwd))
    return {"name": kind, "reads": reads, "target": target, "mode": "HW", "task": "distance", "k": -1, "nwd": nwd}


def two_groups(n_each=600):
    """test 5: a DISTANCE batch of two word groups (three and five words), at least 1,025 slots each, units interleaved"""
    rng = np.random.default_rng(6160)
    T = 40_000
    target = _ACGT[rng.integers(0, 4, T)].copy()
    a = fit_lengths(_reads(target, n_each, 61, 8, M_MIN[3], 96), M_MIN[3], 96, 3)
    c = fit_lengths(_reads(target, n_each, 62, 8, M_MIN[5], 160), M_MIN[5], 160, 5)
    reads = [x for pair in zip(a, c) for x in pair]
    return {"name": "two", "reads": _flip(reads, every=3, first=1), "target": target, "mode": "HW", "task": "distance", "k": -1}


def batch(name):
    """the batch of a child-process test by name"""
    kind, _, arg = name.partition(":")
    if kind == "resolving":
        return seeded_group(int(arg), only_resolving=True)
    if kind == "climbing":
        nwd, _, task = arg.partition(":")
        return seeded_group(int(nwd), only_resolving=False, task=task or "distance")
    if kind == "banded":
        return banded_group(arg)
    if kind == "two":
        return two_groups()
    raise KeyError(name)
