"""CPU: the pair schedule of the bottom-aligned column's `<< 1` (tests/pair_shift_model.py, reads_column_asm.hpp) gives the
same Pn, Mn and score delta as the alignbit chain, for every word count 1..8.

Edge states: every setting of bit 31 and bit 0 of every word (the only bits that cross a word or a pair), with the bits
between all clear and all set.  Up to five words -- the word counts the kernel runs in the pair form -- Ph and Mh go through
the full cross product (4 ** (2 NWD) states, 1,048,576 at five words).  Above that the cross product does not fit (4 ** 16
states at eight words); each vector goes through all of its 4 ** NWD settings while the other walks the same set in another
order, which is exhaustive for the shift itself: Ph and Mh are shifted independently of each other."""
import numpy as np
import pytest

import pair_shift_model as M


def _same(eq, mv, ph, mh):
    a = M.column_tail(eq, mv, ph, mh, M.shift_chain)
    b = M.column_tail(eq, mv, ph, mh, M.shift_pairs)
    for x, y, name in zip(a, b, ("Pn", "Mn", "delta")):
        assert np.array_equal(x, y), name
    assert np.array_equal(M.shift_chain(ph), M.shift_pairs(ph)) and np.array_equal(M.shift_chain(mh), M.shift_pairs(mh))


@pytest.mark.parametrize("nwd", range(1, 9))
def test_edge_bits_of_every_word(nwd):
    rng = np.random.default_rng(900 + nwd)
    for fill_p in (0, 1):
        for fill_m in (0, 1):
            p, m = M.edge_patterns(nwd, fill_p), M.edge_patterns(nwd, fill_m)
            n = len(p)
            if nwd <= 5:
                ph, mh = np.repeat(p, n, axis=0), np.tile(m, (n, 1))
            else:
                walk = (np.arange(n, dtype=np.int64) * 40503 + 12345) % n        # odd multiplier: a permutation of 0..n-1
                assert len(np.unique(walk)) == n
                ph, mh = np.concatenate([p, p[walk]]), np.concatenate([m[walk], m])
            eq = rng.integers(0, 2 ** 32, ph.shape, dtype=np.uint64).astype(np.uint32)
            mv = rng.integers(0, 2 ** 32, ph.shape, dtype=np.uint64).astype(np.uint32)
            _same(eq, mv, ph, mh)


@pytest.mark.parametrize("nwd", range(1, 9))
def test_all_ones_all_zero_and_random(nwd):
    rng = np.random.default_rng(950 + nwd)
    ones, zero = np.full((1, nwd), 0xFFFFFFFF, dtype=np.uint32), np.zeros((1, nwd), dtype=np.uint32)
    for ph in (ones, zero):
        for mh in (ones, zero):
            for eq in (ones, zero):
                for mv in (ones, zero):
                    _same(eq, mv, ph, mh)
    r = [rng.integers(0, 2 ** 32, (10_000, nwd), dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    _same(*r)
    # words that are all ones or all zero at random, so that runs of carries cross several pairs
    r = [np.where(rng.integers(0, 2, (10_000, nwd)) == 1, np.uint32(0xFFFFFFFF), np.uint32(0)) for _ in range(4)]
    _same(*r)


def test_known_values():
    w = np.array([[0x80000000, 0x80000001, 0x00000000, 0xC0000000, 0x00000001]], dtype=np.uint32)
    want = np.array([[0x00000000, 0x00000003, 0x00000001, 0x80000000, 0x00000003]], dtype=np.uint32)
    assert np.array_equal(M.shift_chain(w), want) and np.array_equal(M.shift_pairs(w), want)


@pytest.mark.parametrize("nwd", [3, 5, 7])
def test_lone_word_must_be_shifted_before_its_pair(nwd):
    """the order constraint: the lone last word takes bit 31 of the UNSHIFTED word below it.  Stated input: only bit 31 of
    word NWD - 2 set.  In order, the lone word comes out as 1; fed from the pair after its in-place shift it sees bit 30 of
    that word instead and comes out as 0."""
    w = np.zeros((1, nwd), dtype=np.uint32)
    w[0, nwd - 2] = 0x80000000
    good, bad = M.shift_pairs(w), M.shift_pairs(w, lone_after_pair_shift=True)
    assert np.array_equal(good, M.shift_chain(w)) and good[0, nwd - 1] == 1
    assert bad[0, nwd - 1] == 0 and not np.array_equal(bad, good)
