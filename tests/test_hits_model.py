"""CPU: the definition of a hit (tests/hits_model.py) against the reference, and the two arguments the device
path of hit-list read batches rests on.

  * identity (1): D[j] == edlibAlign(reverse(read), reverse(target[:j+1]), SHW, k = -1).editDistance;
  * identity (2): with r = edlibAlign(read, target, HW, k): r.editDistance == -1 <=> no hit; otherwise the least editDistance
    over the hits equals it, every non-negative end location lies in a hit of that distance, and those hits' numLocations sum
    to the number of non-negative end locations (the reference's -1 location has no counterpart);
  * the seeded argument: for k <= the seed threshold every column with D <= k lies in seed_model.windows(), and the DP
    restarted at each window's first column gives the same hits as the whole row;
  * the stitch rule: segments computed after 2m - 1 warm-up columns, clipped and stitched, give hits(D, k)."""
import numpy as np
import pytest

import hits_model as H
import seed_cases as SC
import seed_model as SM

IUPAC = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]


def _rand(rng, n, alpha):
    return np.ascontiguousarray(rng.choice(np.frombuffer(alpha, dtype=np.uint8), size=n).astype(np.uint8))


def _planted(rng, m, T, alpha):
    """a target with one or two copies of the read carrying a few edits (so that small k finds something)"""
    read, target = _rand(rng, m, alpha), _rand(rng, T, alpha)
    for _ in range(int(rng.integers(0, 3))):
        w = read.copy()
        for _ in range(int(rng.integers(0, 3))):
            w[int(rng.integers(0, m))] = alpha[int(rng.integers(0, len(alpha)))]
        at = int(rng.integers(0, max(1, T - m)))
        target[at:at + len(w)] = w[:T - at]
    return read, target


def _identities(checker, read, target, eq, ks):
    D = H.d_row(read, target, eq)
    rb, tb = read.tobytes(), target.tobytes()
    for j in range(len(target)):                                           # (1)
        got = checker.align(rb[::-1], tb[:j + 1][::-1], "SHW", "distance", -1, eq)["editDistance"]
        assert got == D[j], (j, got, D[j])
    assert D.max() <= len(read)
    for k in ks:                                                           # (2)
        hs = H.hits(D, k)
        r = checker.align(rb, tb, "HW", "distance", k, eq)
        if r["editDistance"] == -1:
            assert hs == [], (k, hs)
            continue
        assert hs and min(h[2] for h in hs) == r["editDistance"], (k, hs, r)
        ends = [e for e in r["endLocations"] if e >= 0]
        best = [h for h in hs if h[2] == r["editDistance"]]
        for e in ends:
            assert any(h[0] <= e <= h[1] for h in best), (k, e, hs)
        assert sum(h[4] for h in best) == len(ends), (k, hs, r)
        for f, l, ed, pos, cnt in hs:                                      # the definition itself
            assert (f == 0 or D[f - 1] > k) and (l == len(D) - 1 or D[l + 1] > k) and D[f:l + 1].max() <= k
            assert ed == D[f:l + 1].min() == D[pos] and (D[f:pos] > ed).all() and cnt == np.count_nonzero(D[f:l + 1] == ed)


@pytest.mark.parametrize("seed", range(12))
def test_model_matches_reference_on_random_cases(checker, seed):
    rng = np.random.default_rng(4100 + seed)
    for _ in range(5):
        alpha = b"ACGTN"[:int(rng.integers(1, 6))]
        m, T = int(rng.integers(1, 40)), int(rng.integers(30, 400))
        read, target = _planted(rng, m, T, alpha)
        _identities(checker, read, target, None, range(0, m + 3))


@pytest.mark.parametrize("seed", range(4))
def test_model_matches_reference_with_equalities(checker, seed):
    rng = np.random.default_rng(4200 + seed)
    for _ in range(4):
        m, T = int(rng.integers(1, 40)), int(rng.integers(30, 300))
        read, target = _planted(rng, m, T, b"ACGTRYN")
        _identities(checker, read, target, IUPAC, range(0, m + 3))


def test_consequences_of_the_definition():
    read, target = np.frombuffer(b"ACGTAC", dtype=np.uint8), np.frombuffer(b"TTACGTACTTTTACGAACTT", dtype=np.uint8)
    D = H.d_row(read, target)
    assert H.hits(D, len(read)) == [(0, len(target) - 1, 0, 7, 1)]           # k >= m: one hit over everything
    assert H.hits(D, len(read) + 5) == H.hits(D, len(read))
    assert H.hits(D, 0) == [(7, 7, 0, 7, 1)]
    assert [h[:3] for h in H.hits(D, 1)] == [(6, 8, 0), (17, 17, 1)]    # ACGAAC ends at column 17: one substitution
    withn = np.frombuffer(b"ACNTAC", dtype=np.uint8)                          # a byte the target lacks can still hit
    assert [h[2] for h in H.hits(H.d_row(withn, target), 1)] == [1]
    assert H.hits(H.d_row(np.frombuffer(b"GGGGGG", dtype=np.uint8), target), 2) == []


@pytest.mark.parametrize("seed", range(6))
def test_bit_vector_rows_match_the_textbook_rows(seed):
    rng = np.random.default_rng(4300 + seed)
    alpha = b"ACGTRYN"[:int(rng.integers(1, 8))]
    eq = IUPAC if seed % 2 else None
    target = _rand(rng, int(rng.integers(1, 500)), alpha)
    reads = [_rand(rng, m, alpha + b"X") for m in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256)]
    rows = H.d_rows(reads, target, eq)
    for i, r in enumerate(reads):
        assert np.array_equal(rows[i], H.d_row(r, target, eq)), (seed, len(r))
    own = np.stack([np.roll(target, i) for i in range(len(reads))])           # a target row per read
    rows = H.d_rows(reads, own, eq)
    for i, r in enumerate(reads):
        assert np.array_equal(rows[i], H.d_row(r, own[i], eq)), (seed, len(r))
    for k in (0, 2, 9, 300):
        c = H.hits_csr(rows, k)
        for i in range(len(reads)):
            s, e = c["unitOffsets"][i], c["unitOffsets"][i + 1]
            got = list(zip(*(c[f][s:e].tolist() for f in ("firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations"))))
            assert got == H.hits(rows[i], k), (seed, i, k)


# ------------------------------------------------------------------------------------------------- the seeded argument

@pytest.mark.parametrize("nwd,k", [(1, 0), (1, 1), (2, 3), (3, 2), (4, 5), (5, 8), (8, 6)])
def test_seed_windows_hold_every_hit_and_restarts_change_nothing(nwd, k):
    span = 32 * nwd + 2 * k + 2
    P = SC.Planter(nwd, 2 * SC.RESERVE + 150 * span, k, 4400 + 10 * nwd + k).plant(over_caps=False)
    target = P.target
    T = len(target)
    m_min = min(len(r) for r in P.reads)
    assert m_min // (k + 1) >= SM.Q                                           # pieces a seed pass at k can look up
    index = SM.build_index(target.tobytes(), SM.Q)
    some = 0
    for read in P.reads[::2 if nwd >= 5 else 1]:
        m = len(read)
        D = H.d_row(read, target)
        for kk in sorted({0, k // 2, k}):
            diags = SM.lookup(read, target.tobytes(), kk, index=index, caps=False)
            ws = SM.windows(diags, m, kk, T)
            inside = np.zeros(T, dtype=bool)
            for a, b in ws:
                inside[a:b + 1] = True
            assert not (D[~inside] <= kk).any(), (m, kk)
            got = []
            for a, b in ws:                                                   # restarted at the window's first column
                got += [(f + a, l + a, ed, pos + a, cnt) for f, l, ed, pos, cnt in H.hits(H.d_row(read, target[a:b + 1]), kk)]
            want = H.hits(D, kk)
            assert got == want, (m, kk)
            some += len(want)
    assert some >= len(P.reads) // 2                                          # (the planted reads are found)


# ------------------------------------------------------------------------------------------------------ the stitch rule

def _segmented(read, target, k, seglen):
    """the device's plan: [0, T) in segments, each computed after 2m - 1 warm-up columns that record nothing, runs clipped
    to the segment, then stitched"""
    m, T = len(read), len(target)
    runs = []
    for c0 in range(0, T, seglen):
        c1 = min(T, c0 + seglen)
        cw = max(0, c0 - (2 * m - 1))
        D = H.d_row(read, target[cw:c1])[c0 - cw:]
        runs += [(f + c0, l + c0, ed, pos + c0, cnt) for f, l, ed, pos, cnt in H.hits(D, k)]
    return H.stitch(runs)


@pytest.mark.parametrize("seed", range(8))
def test_segments_clipped_and_stitched_equal_the_whole_row(seed):
    rng = np.random.default_rng(4500 + seed)
    alpha = b"ACGT"[:int(rng.integers(1, 5))]
    m = int(rng.integers(1, 40))
    read, target = _planted(rng, m, int(rng.integers(200, 700)), alpha)
    D = H.d_row(read, target)
    for k in sorted({0, 1, m // 4, m // 2, m, m + 2}):
        for seglen in (16, 48, 112):
            assert _segmented(read, target, k, seglen) == H.hits(D, k), (seed, k, seglen)


def test_stitch_across_whole_segments_and_equal_minima():
    read = np.frombuffer(b"AAAAAAAA", dtype=np.uint8)
    target = np.frombuffer(b"A" * 200, dtype=np.uint8)
    D = H.d_row(read, target)
    for k in (0, 2, 8):                                                       # one run [m - 1 - k, T - 1] over 13 segments
        want = H.hits(D, k)
        assert want == [(7 - k if k < 8 else 0, 199, 0, 7, 193)]
        assert _segmented(read, target, k, 16) == want
    read = np.frombuffer(b"ACGTACGT", dtype=np.uint8)                         # period 4: the least value on both sides of a cut
    target = np.frombuffer(b"ACGT" * 40, dtype=np.uint8)
    D = H.d_row(read, target)
    for k in (0, 1, 3):
        for seglen in (16, 32):
            assert _segmented(read, target, k, seglen) == H.hits(D, k), (k, seglen)
    # the parts of a stitched run: a lower least value on the right replaces, an equal one adds, a higher one only extends
    assert H.stitch([(0, 3, 2, 1, 2), (4, 7, 1, 5, 1), (8, 9, 1, 8, 2), (10, 12, 3, 10, 1), (20, 21, 0, 20, 1)]) == \
        [(0, 12, 1, 5, 3), (20, 21, 0, 20, 1)]
