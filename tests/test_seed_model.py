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
