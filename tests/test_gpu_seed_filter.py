"""-m gpu: the exact k-mer seed filter that replaces the banded first pass of HW read groups against a target of at most four
symbols (edlib_amd/csrc/reads_seed.hip; the argument is tests/seed_model.py).  Every batch is compared with
the reference on every field.  The batches that take the new path prove it through the work counter: the banded first pass
computes at least one word per column per read, so word_steps stays below nslots x T only when the seeds did the first pass.
"""
import numpy as np
import pytest

from edlib_amd import synth
from seed_model import seed_threshold
from test_gpu_long_reads import _check

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _nslots(n):
    return (n + 63) // 64 * 64


def _mutate(rng, w, edits, at):
    """`edits` edits of w at the query positions `at` (cycled), kinds cycling substitution / insertion / deletion"""
    w = w.copy()
    for e in range(edits):
        p = int(min(max(at[e % len(at)], 0), len(w) - 1))
        kind = (e + int(rng.integers(0, 3))) % 3
        if kind == 0:
            w[p] = _ACGT[(np.searchsorted(_ACGT, w[p]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            w = np.insert(w, p, _ACGT[rng.integers(0, 4)])
        else:
            w = np.delete(w, p)
    return np.ascontiguousarray(w)


def _reads(target, n, seed, kf, mlo=131, mhi=158, unrelated=0.05, above=0.03, with_n=0.02):
    """n reads of mlo..mhi bases: copies of the target with 0..kf edits, many on the boundaries of the kf + 1 pieces, on
    the first and the last base and as indels at both ends; `above` of them with kf + 1 or kf + 2 edits, `unrelated` of
    them random, `with_n` of them holding an N; reads at the target's first and last columns"""
    rng = np.random.default_rng(seed)
    T = len(target)
    out = []
    for i in range(n):
        m = int(rng.integers(mlo, mhi + 1))
        u = rng.random()
        if u < unrelated:
            out.append(np.ascontiguousarray(_ACGT[rng.integers(0, 4, m)]))
            continue
        s = 0 if i % 97 == 0 else (T - m if i % 97 == 1 else int(rng.integers(0, T - m)))
        w = target[s:s + m]
        edits = int(rng.integers(kf + 1, kf + 3)) if u < unrelated + above else int(rng.integers(0, kf + 1))
        L = m // (kf + 1)
        bounds = [j * L for j in range(1, kf + 1)] + [j * L - 1 for j in range(1, kf + 1)]
        style = i % 4
        if style == 0:
            at = bounds
        elif style == 1:
            at = [0, m - 1] + bounds
        elif style == 2:
            at = [0, m - 1]
        else:
            at = list(rng.integers(0, m, max(1, edits)))
        rng.shuffle(at)
        w = _mutate(rng, w, edits, at)
        if rng.random() < with_n:
            w = w.copy()
            w[int(rng.integers(0, len(w)))] = ord("N")
        out.append(w)
    return out


def test_seed_batch_a(engine):
    """16,384 reads of 129..160 bases against 256 kb: one group of five words"""
    target = synth.random_dna(801, 256_000)
    kf = seed_threshold(129, len(target))
    assert kf == 8
    reads = _reads(target, 16_384, 802, kf)
    reads[0] = np.ascontiguousarray(target[:129])                      # shortest and longest reads at both ends
    reads[1] = np.ascontiguousarray(target[-160:])
    reads[2] = np.ascontiguousarray(np.concatenate([_ACGT[[0, 1, 2]], target[:140]]))   # hanging over the first column
    reads[3] = np.ascontiguousarray(np.concatenate([target[-140:], _ACGT[[3, 2]]]))     # and over the last
    st = _check(engine, reads, target, "distance")
    assert st["path"] & 1
    assert st["word_steps"] < _nslots(len(reads)) * len(target), st


def test_seed_repeats_exact_pass_and_hand_back(engine):
    """a 150-base block copied 20 times (more than 16 end locations: the exact pass) and another copied 100 times (past the
    bucket cap: handed back to the banded scan)"""
    rng = np.random.default_rng(811)
    T = 256_000
    target = synth.random_dna(812, T).copy()
    blocks = [synth.random_dna(813, 150), synth.random_dna(814, 150)]
    starts = rng.choice(np.arange(0, T - 150, 160), 120, replace=False)
    for j, at in enumerate(starts):
        target[at:at + 150] = blocks[0 if j < 20 else 1]
    kf = seed_threshold(150, T)
    reads = _reads(target, 8_192, 815, kf, mlo=150, mhi=150, unrelated=0.02, above=0.0, with_n=0.0)
    for b in blocks:
        for e in range(6):
            reads.append(_mutate(rng, b, e, [int(x) for x in rng.integers(0, 150, 6)]) if e else np.ascontiguousarray(b))
    st = _check(engine, reads, target, "distance")
    assert st["overflow_units"] >= 1, st
    assert st["word_steps"] < _nslots(len(reads)) * T, st


@pytest.mark.parametrize("k", [3, 20])
def test_seed_caller_k(engine, k):
    target = synth.random_dna(821, 256_000)
    kf = seed_threshold(131, len(target))
    reads = _reads(target, 8_192, 822 + k, kf)
    st = _check(engine, reads, target, "distance", k=k)
    assert st["word_steps"] < _nslots(len(reads)) * len(target), st


def test_five_symbol_target_keeps_banded_pass(engine):
    """ACGTN: not the new path (more than four symbols); the banded first pass computes >= one word per column per read"""
    target = synth.random_dna(831, 256_000).copy()
    target[np.random.default_rng(832).integers(0, len(target), 300)] = ord("N")
    reads = _reads(target, 8_192, 833, seed_threshold(131, len(target)))
    st = _check(engine, reads, target, "distance")
    assert st["word_steps"] >= _nslots(len(reads)) * len(target), st
