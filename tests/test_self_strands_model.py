"""CPU: the host statements of a both-strand self batch -- self_strands_model() on hand-made vectors, and the complement
condition under which the self kernel may reverse-complement either sequence of a pair, restated in numpy
(complement_symmetric(): the specification the GPU tests route by)."""
import numpy as np

import edlib_amd

IUPAC_CLOSED = [("R", "A"), ("R", "G"), ("Y", "C"), ("Y", "T"), ("N", "A"), ("N", "C"), ("N", "G"), ("N", "T")]


def complement(b):
    """The complement of one byte value (edlibAmdReverseComplement on one byte)."""
    return edlib_amd.reverse_complement(bytes([b]))[0]


def match_table(eqs):
    """Eq [256][256]: identity plus the additional equalities, both directions."""
    eq = np.eye(256, dtype=bool)
    for pair in eqs or []:
        a, b = ((x if isinstance(x, bytes) else x.encode("latin-1"))[0] for x in pair)
        eq[a, b] = eq[b, a] = True
    return eq


def complement_symmetric(present, eqs=None):
    """Eq(c(x), y) <=> Eq(x, c(y)) for all bytes x, y of `present`: NW(revcomp(a), b) == NW(revcomp(b), a) for all
    sequences over them, so a both-strand self batch may take such a set on its kernel."""
    p = np.array(sorted(set(bytes(present))), dtype=np.int64)
    if len(p) == 0:
        return True
    c = np.array([complement(int(b)) for b in p], dtype=np.int64)
    eq = match_table(eqs)
    return bool(np.array_equal(eq[c[:, None], p[None, :]], eq[p[:, None], c[None, :]]))


def test_reverse_complement_bytes():
    assert complement(ord("A")) == ord("T") and complement(ord("U")) == ord("A") and complement(ord("n")) == ord("n")
    assert complement(ord("r")) == ord("y") and complement(ord("#")) == ord("#")


def test_self_strands_model_hand_made():
    #      tie   fwd   rev   none  only fwd  only rev  tie at 0
    fwd = [3,    1,    5,    -1,   2,        -1,       0]
    rev = [3,    4,    2,    -1,   -1,       6,        0]
    ed, strand = edlib_amd.self_strands_model(fwd, rev)
    assert ed.dtype == np.int32 and strand.dtype == np.uint8
    assert ed.tolist() == [3, 1, 2, -1, 2, 6, 0]
    assert strand.tolist() == [2, 0, 1, 0, 0, 1, 2]          # ties go forward with bit 1; bit 0 only where rev is better
    ed, strand = edlib_amd.self_strands_model([], [])
    assert ed.shape == (0,) and strand.shape == (0,)


def test_self_strands_model_is_the_cross_rule():
    rng = np.random.default_rng(3)
    fwd, rev = rng.integers(-1, 5, size=500), rng.integers(-1, 5, size=500)
    ed, strand = edlib_amd.self_strands_model(fwd, rev)
    for f, r, e, s in zip(fwd.tolist(), rev.tolist(), ed.tolist(), strand.tolist()):
        if f >= 0 and (r < 0 or f <= r):
            assert (e, s) == (f, 2 if f == r else 0)
        elif r >= 0:
            assert (e, s) == (r, 1)
        else:
            assert (e, s) == (-1, 0)


def test_complement_condition():
    assert complement_symmetric(b"ACGT")
    assert complement_symmetric(b"ACGTNacgtn")
    assert complement_symmetric(b"ACGTRYN", IUPAC_CLOSED)
    assert complement_symmetric(b"ACGTRYKMSWBDHVN")
    assert not complement_symmetric(b"ACGU")                  # c(U) = A, c(A) = T
    assert not complement_symmetric(b"acgu")
    assert complement_symmetric(b"CGU")                       # without A or T present nothing tells U from T
    assert not complement_symmetric(b"ACGTR", [("R", "A")])   # (R, A) without (Y, T)
    assert complement_symmetric(b"ACGTRY", [("R", "A"), ("Y", "T")])
    assert complement_symmetric(b"")
