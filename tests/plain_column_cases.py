"""Batches of tests/test_gpu_plain_column.py, built the same way by the test and by its child process
(tests/plain_column_child.py).  All are HW, distance, k = -1 against a target of T = 70,001 symbols (not a multiple of 16: the
last segment of a scan ends in the ragged-tail loop; above 65,536: the last level's 4,096-column pre-scan runs) and leave at
least 4,096 reads open for the last level, which then takes the plain full-height kernel on bottom-aligned rows."""
import numpy as np

T = 70_001
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

N_READS_B = {nwd: 7488 if nwd == 1 else 4160 for nwd in range(1, 9)}
NAMES = ["A"] + ["B%d" % n for n in range(1, 9)]


def _random(rng, n):
    return _ACGT[rng.integers(0, 4, n)]


def _edit(rng, w, nedit):
    """nedit substitutions, insertions and deletions, drawn one after the other"""
    w = w.copy()
    for _ in range(nedit):
        p = int(rng.integers(0, len(w)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            w[p] = _ACGT[(int(np.searchsorted(_ACGT, w[p])) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1 and len(w) > 130:
            w = np.delete(w, p)
        else:
            w = np.insert(w, p, _ACGT[rng.integers(0, 4)])
    return np.ascontiguousarray(w)


def batch_a():
    """4,096 uniform random reads, lengths cycling over 129..160 (every pad 0..31 of the five-word group), and 64 reads
    planted with 12..40 edits: windows anywhere, one that starts at column 0, one that ends at column T - 1, and one whose
    window stands 20 times in the target (more end locations than a slot's 16 positions)"""
    rng = np.random.default_rng(4101)
    target = _random(rng, T)
    motif = _random(rng, 150)
    for i in range(20):                                   # 20 copies, well apart, clear of both ends
        s = 3_000 + 3_200 * i
        target[s:s + 150] = motif
    reads = [_random(rng, 129 + i % 32) for i in range(4096)]
    planted = [_edit(rng, target[0:150], 14), _edit(rng, target[T - 150:T], 13), _edit(rng, motif, 12)]
    for i in range(61):
        m = 132 + int(rng.integers(0, 25))
        s = int(rng.integers(0, T - m))
        planted.append(_edit(rng, target[s:s + m], 12 + i % 29))
    for r in planted:
        assert 129 <= len(r) <= 160, len(r)
    # planted reads spread through the batch rather than in a block of their own
    for i, r in enumerate(planted):
        reads.insert(65 * i + 7, r)
    assert len(reads) == 4160
    return {"reads": reads, "target": target}


def batch_b(nwd):
    """4,160 uniform random reads of 32 nwd - 20, 32 nwd - 1 and 32 nwd symbols in turn: one group of nwd words.
    One word takes 7,488: a random 12-mer always occurs within 3 edits in 70,001 columns and a third of the 31- and 32-mers
    within 8, so they resolve at the first level (threshold 8) -- of 4,160 reads only 2,630 would reach the last level, and
    below 4,096 it does not take the plain kernel at all; of 7,488 about 4,700 do."""
    rng = np.random.default_rng(4200 + nwd)
    target = _random(rng, T)
    lengths = (32 * nwd - 20, 32 * nwd - 1, 32 * nwd)
    reads = [_random(rng, lengths[i % 3]) for i in range(N_READS_B[nwd])]
    return {"reads": reads, "target": target}


def batch(name):
    return batch_a() if name == "A" else batch_b(int(name[1:]))
