"""The argument of the exact k-mer seed filter (tests/seed_model.py, edlib_amd/csrc/reads_seed.hip) against the textbook DP:
pigeonhole over k + 1 exact pieces, windows of +-k around each diagonal, merging, restarted verification.  Whenever the
DP's best is <= k the filter gives that best and the full list of end columns; otherwise it says "unresolved"."""
import numpy as np
import pytest

import seed_model as SM

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _edit(rng, w, at, kind):
    w = w.copy()
    at = int(min(max(at, 0), len(w) - 1))
    if kind == 0:
        c = w[at]
        w[at] = _ACGT[(int(np.searchsorted(_ACGT, c)) + 1 + int(rng.integers(0, 3))) % 4] if c in _ACGT else _ACGT[0]
    elif kind == 1:
        w = np.insert(w, at, _ACGT[rng.integers(0, 4)])
    else:
        w = np.delete(w, at)
    return w


def _check(qr, t, k, q, caps=False):
    got = SM.seed_filter(qr, t, k, q=q, caps=caps)
    want = SM.reference(qr, t, k)
    if got == "back":
        return "back"
    if want is None:
        assert got is None, (got, qr.tobytes(), t.tobytes(), k)
    else:
        assert got is not None, (want, qr.tobytes(), t.tobytes(), k)
        assert got[0] == want[0] and got[1] == want[1], (got, want, qr.tobytes(), t.tobytes(), k)
    return "ok"


def test_seed_threshold_values():
    assert SM.seed_threshold(150, 5_000_000) == 9          # config 2: ten pieces of 15 bases
    assert SM.seed_threshold(129, 256_000) == 8
    assert SM.seed_threshold(150, 256_000) == 10
    assert SM.seed_threshold(11, 5_000_000) == -1          # pieces below 12 symbols
    assert SM.seed_threshold(40, 5_000_000) == 1
    for m, T in [(150, 5_000_000), (129, 256_000), (256, 3_000_000_000)]:
        k = SM.seed_threshold(m, T)
        L = m // (k + 1)
        assert L >= 12 and (k + 1) * T / 4 ** L <= 1 / 8
        if k < 16:
            L2 = m // (k + 2)
            assert L2 < 12 or (k + 2) * T / 4 ** L2 > 1 / 8


def test_pieces_cover_the_read():
    for m in range(1, 300):
        for k in range(0, 17):
            ps = SM.pieces(m, k)
            assert len(ps) == k + 1 and ps[0][0] == 0 and sum(n for _, n in ps) == m
            assert all(ps[i][0] + ps[i][1] == ps[i + 1][0] for i in range(k))
            assert all(n >= m // (k + 1) for _, n in ps)


def test_windows_merge_sorted_disjoint():
    ws = SM.windows([-3, 0, 2, 40, 41, 200], 20, 2, 210)
    assert ws == [(0, 23), (38, 62), (198, 209)]


@pytest.mark.parametrize("seed", range(8))
def test_edits_on_piece_boundaries_and_ends(seed):
    """exactly k and k + 1 edits, on every piece boundary, on the first and the last base, indels at both ends"""
    rng = np.random.default_rng(1000 + seed)
    n = 0
    for case in range(40):
        T = int(rng.integers(120, 260))
        t = _ACGT[rng.integers(0, 4, T)]
        k = int(rng.integers(0, 5))
        q = 3
        m = int(rng.integers(max(q * (k + 1), 8), 48))
        s = int(rng.integers(0, T - m + 1)) if case % 5 else (0 if case % 10 == 0 else T - m)
        w = t[s:s + m].copy()
        bounds = [o for o, _ in SM.pieces(m, k)][1:]
        spots = sorted(set(bounds + [b - 1 for b in bounds] + [0, m - 1]))
        for edits in (k, k + 1):
            for style in range(3):
                r = w.copy()
                for e in range(edits):
                    if style == 0:
                        at, kind = spots[(e * 7 + case) % len(spots)], e % 3
                    elif style == 1:
                        at, kind = (0 if e % 2 == 0 else len(r) - 1), 1 + e % 2     # indels at both ends
                    else:
                        at, kind = (0 if e % 2 == 0 else len(r) - 1), 0
                    r = _edit(rng, r, at, kind)
                if len(r) >= q * (k + 1):
                    assert _check(r, t, k, q) == "ok"
                    n += 1
    assert n >= 200


@pytest.mark.parametrize("seed", range(6))
def test_random_cases(seed):
    """random reads: planted with 0..k+2 edits, unrelated, tandem repeats, several copies, bytes absent from the target"""
    rng = np.random.default_rng(2000 + seed)
    n = 0
    for case in range(60):
        kind = case % 6
        T = int(rng.integers(100, 320))
        if kind == 2:                                          # tandem repeat target
            unit = _ACGT[rng.integers(0, 4, int(rng.integers(1, 6)))]
            t = np.resize(unit, T).copy()
            t[rng.integers(0, T, 4)] = _ACGT[rng.integers(0, 4, 4)]
        else:
            t = _ACGT[rng.integers(0, 4, T)]
        k = int(rng.integers(0, 6))
        q = int(rng.integers(2, 5))
        m = int(rng.integers(q * (k + 1), q * (k + 1) + 30))
        if m >= T:
            continue
        s = int(rng.integers(0, T - m + 1))
        if kind == 3:                                          # several copies of one block
            for at in rng.integers(0, T - m + 1, 3):
                t[at:at + m] = t[s:s + m]
        r = t[s:s + m].copy()
        if kind == 1:
            r = _ACGT[rng.integers(0, 4, m)]
        for _ in range(int(rng.integers(0, k + 3))):
            r = _edit(rng, r, int(rng.integers(0, len(r))), int(rng.integers(0, 3)))
        if kind == 4:                                          # a byte absent from the target
            r = r.copy(); r[int(rng.integers(0, len(r)))] = ord("N")
        if kind == 5:                                          # a target of three symbols, a query byte it lacks
            t = np.where(t == ord("T"), ord("A"), t).astype(np.uint8)
        if len(r) < q * (k + 1):
            continue
        assert _check(r, t, k, q) == "ok"
        n += 1
    assert n >= 40


def test_at_least_2000_cases_in_total():
    """2,000 more planted reads with 0 .. k + 2 edits on short targets"""
    rng = np.random.default_rng(3000)
    n = 0
    while n < 2000:
        T = int(rng.integers(40, 90))
        t = _ACGT[rng.integers(0, 4, T)]
        k = int(rng.integers(0, 4)); q = 2
        m = int(rng.integers(q * (k + 1), min(T, q * (k + 1) + 16)))
        s = int(rng.integers(0, T - m + 1))
        r = t[s:s + m].copy()
        for _ in range(int(rng.integers(0, k + 3))):
            r = _edit(rng, r, int(rng.integers(0, len(r))), int(rng.integers(0, 3)))
        if len(r) < q * (k + 1):
            continue
        assert _check(r, t, k, q) == "ok"
        n += 1


def test_caps_only_hand_back():
    """with the kernel's caps a read is either handed back or answered exactly; 100 copies of a block hand it back,
    20 do not"""
    rng = np.random.default_rng(4000)
    block = _ACGT[rng.integers(0, 4, 150)]
    for copies, want in ((20, "ok"), (100, "back")):
        t = _ACGT[rng.integers(0, 4, 400 * copies + 500)].copy()
        for j in range(copies):
            t[400 * j:400 * j + 150] = block
        got = SM.seed_filter(block, t, 9, q=12, caps=True)
        if want == "back":
            assert got == "back"
        else:
            assert got != "back" and got[0] == 0 and len(got[1]) == copies
            assert got == SM.reference(block, t, 9)


# ------------------------------------------------------------------------------ the planted inputs of tests/seed_cases.py
# (shared with tests/test_gpu_seed_filter.py): on a target of a few thousand columns, with q = 12 as in the kernel, every
# generator does what it claims -- predict() gives the claimed diagonals / columns / bucket / window / hand-back -- and every
# read that is not handed back gets the textbook DP's answer from the filter with the caps on.

import seed_cases as SC

# (word count, k): k_f of the GPU batches at T = 256,000, k = 0 (one piece = the whole read), and the pairs that give piece
# lengths 12 / 13 (1, 1), 27 .. 29 (1, 0: lengths 12 .. 32) and 43 / 44 (3, 1)
_PLANTED = [(1, 1), (2, 3), (3, 5), (4, 7), (5, 8), (6, 11), (7, 13), (8, 16), (1, 0), (4, 0), (8, 0), (4, 1), (8, 1), (4, 6),
            (8, 15), (3, 1)]


def test_seed_thresholds_of_the_gpu_batches():
    assert [SM.seed_threshold(SC.M_MIN[w], 256_000) for w in range(1, 9)] == [1, 3, 5, 7, 8, 11, 13, 16]
    for w in range(1, 9):                                     # the same at T mod 16 = 1 and 15
        assert SM.seed_threshold(SC.M_MIN[w], 256_001) == SM.seed_threshold(SC.M_MIN[w], 255_999) == SM.seed_threshold(SC.M_MIN[w], 256_000)
    assert SM.seed_threshold(108, 200_000) == 8 and SM.seed_threshold(108, 256_000) == 7
    assert SM.seed_threshold(97, 256_000) == 7 and SM.seed_threshold(12, 256_000) == 0


def test_piece_lengths_reach_every_compare_tail():
    """len - 12 in {0, 1, 15, 16, 17, 31, 32} over the (word count, k) pairs of the GPU tests"""
    seen = set()
    for nwd, k in _PLANTED:
        mlo = max(32 * (nwd - 1) + 1, 12 * (k + 1)) if (nwd, k) not in ((1, 1), (2, 3), (3, 5), (4, 7)) else SC.M_MIN[nwd]
        for m in range(mlo, 32 * nwd + 1):
            seen |= {n - 12 for _, n in SM.pieces(m, k)}
    assert {0, 1, 15, 16, 17, 31, 32} <= seen


@pytest.mark.parametrize("gen", SC.GENERATORS)
@pytest.mark.parametrize("nwd,k", _PLANTED)
def test_planted_generator_does_what_it_claims(nwd, k, gen):
    span = 32 * nwd + 2 * k + 2
    T = 2 * SC.RESERVE + (48 * span if gen.startswith("diag") else 100 * span if gen == "compare_tails" else max(2_000, 14 * span))
    T = T // 16 * 16 + (0, 1, 15)[(nwd + k) % 3]
    P = SC.Planter(nwd, T, k, 500 + 17 * nwd + k)
    getattr(P, gen)()
    assert len(P.reads) >= (0 if (nwd, k, gen) == (1, 0, "window_1025") else 1) and len(P.target) == T and set(P.target.tolist()) <= set(b"ACGT")
    tb = P.target.tobytes()
    index, present = SM.build_index(tb, SM.Q), set(tb)
    pred = [SM.predict(r, tb, k, index, present) for r in P.reads]
    assert SC.claims_hold(P.claims, pred) == []
    for r, c, p in zip(P.reads, P.claims, pred):
        want = SM.reference(r, P.target, k)
        if "found" in c:
            assert (want is not None) == c["found"], (c, want)
        if "dist" in c:
            assert want[0] == c["dist"], (c, want)
        got = SM.seed_filter(r, P.target, k, index=index, caps=True)
        assert (got == "back") == p["back"]
        if not p["back"]:
            assert got == want, (c, got, want)


def test_caps_sit_on_both_sides():
    """32 / 33 diagonals, buckets of 64 / 65, windows of 1024 / 1025 columns: exactly, for a short and a long word count"""
    for nwd, k in ((2, 3), (8, 16)):
        P = SC.Planter(nwd, 2 * SC.RESERVE + 200 * (32 * nwd + 2 * k + 2), k, 600 + nwd)
        for gen in ("diag_32", "diag_33", "bucket_64", "bucket_65", "window_1024", "window_1025"):
            getattr(P, gen)()
        pred = SM.predict_batch(P.reads, P.target, k)
        assert [p["back"] for p in pred] == [False, True, False, True, False, True]
        assert pred[0]["diagonals"] == 32 and pred[2]["bucket"] == 64 and pred[3]["bucket"] == 65
        assert pred[4]["window"] == 1024 and pred[4]["diagonals"] >= 4 and pred[5]["window"] == 1025


def test_predict_is_lookup_and_windows():
    rng = np.random.default_rng(700)
    t = _ACGT[rng.integers(0, 4, 3000)]
    r = t[100:160].copy()
    p = SM.predict(r, t, 3, SM.build_index(t, SM.Q))
    assert p == {"back": False, "diagonals": 1, "columns": 66, "bucket": 1, "window": 66}
    assert SM.predict(r[:40], t, 3, SM.build_index(t, SM.Q))["back"]          # pieces of 10 symbols


@pytest.mark.parametrize("nwd", [1, 5, 8])
def test_gpu_batches_keep_their_claims_at_full_size(nwd):
    """the batches of the GPU tests (256,000 columns, no DP here): the model hands back nothing in the work-accounting batch
    and exactly the three over-the-cap reads in the caps batch; the planted claims hold there too"""
    k = SM.seed_threshold(SC.M_MIN[nwd], 256_000)
    b = SC.single_group(nwd, k, mlo=SC.M_MIN[nwd])
    pred = SM.predict_batch(b["reads"], b["target"], k)
    assert sum(p["back"] for p in pred) == 0
    b = SC.batch("caps:%d" % nwd)
    pred = SM.predict_batch(b["reads"], b["target"], k)
    assert SC.claims_hold(b["claims"], pred, keys=("back",)) == []        # (a random extra hit may add a diagonal here)
    caps = [(c, p) for c, p in zip(b["claims"], pred) if c and (c.get("bucket", 0) >= 64 or c.get("window") or c.get("diagonals", 0) >= 32 or c["back"])]
    assert len(caps) == 6 and SC.claims_hold([c for c, _ in caps], [p for _, p in caps]) == []
    assert sum(p["back"] for p in pred) == sum(1 for c in b["claims"] if c and c["back"]) == 3


@pytest.mark.parametrize("name", ["three_symbols", "two_symbols", "low_complexity"])
def test_small_alphabet_batches_on_a_small_target(name):
    """the same generators at 6,000 columns: the alphabet is what the name says, and every read the model does not hand back
    gets the textbook DP's answer (a read holding a base the target lacks included)"""
    b = getattr(SC, name)(nwd=2, k=3, T=6_000, n=48, seed=800)
    t = b["target"]
    assert len(set(t.tolist())) == {"three_symbols": 3, "two_symbols": 2, "low_complexity": 4}[name]
    if name == "three_symbols":
        assert sum(1 for r in b["reads"] if ord("T") in r.tolist()) >= 16
    index = SM.build_index(t, SM.Q)
    back = 0
    for r in b["reads"]:
        got = SM.seed_filter(r, t, 3, index=index, caps=True)
        assert (got == "back") == SM.predict(r, t, 3, index)["back"]
        back += got == "back"
        if got != "back":
            assert got == SM.reference(r, t, 3)
    if name == "low_complexity":
        assert 0 < back < len(b["reads"])                     # (the run and the repeat overflow a bucket, the rest does not)


def test_two_symbol_buckets_straddle_the_cap_at_full_size():
    """256,000 columns of two symbols: 4096 keys occur, about 62.5 positions each -- both sides of the cap of 64"""
    b = SC.two_symbols()
    sizes = np.array([len(v) for v in SM.build_index(b["target"], SM.Q).values()])
    assert len(sizes) == 4096 and 55 < sizes.mean() < 70
    assert (sizes > SM.BUCKET_CAP).sum() > 400 and (sizes <= SM.BUCKET_CAP).sum() > 400
