"""Shared by the grouped self-batch tests (test_self_groups_model.py on the CPU, test_gpu_self_groups.py on the device):
the counters of a grouped self batch as numpy functions, the same-group pair list, and the planted inputs -- the group
sizes 1, 2, 3, 7, 8, 9, 63, 64, 65 with interleaved labels, one group of 1,500 among singletons, and 200-base sequences
scattered through short ones (the cases tests/self_groups_host.cpp runs through the layout on the host)."""
import numpy as np

from edlib_amd import grouped_hits_model  # noqa: F401  (the index mapping, stated beside the other models)
from test_self_model import self_cells, self_word_steps

SIZES = (1, 2, 3, 7, 8, 9, 63, 64, 65)
LABELS = (5, -7, 0, 2**31 - 1, -2**31, 11, -1, 3, 1)


def members_of(groups):
    """{label: ascending indices} of a label array."""
    g = np.asarray(groups).reshape(-1)
    order = np.argsort(g, kind="stable")
    cut = np.flatnonzero(np.diff(g[order])) + 1
    return {int(g[part[0]]): part for part in np.split(order, cut) if len(part)}


def grouped_cells(lengths, groups):
    """Stats.cells of a grouped self batch: per group the sum of m_i * m_j over i < j."""
    m = np.asarray(lengths, dtype=np.int64)
    return sum(self_cells(m[part]) for part in members_of(groups).values())


def grouped_word_steps(lengths, groups, k):
    """Stats.word_steps of a grouped self batch over at most 16 symbols: per group, a self batch's."""
    m = np.asarray(lengths, dtype=np.int64)
    return sum(self_word_steps(m[part], k) for part in members_of(groups).values())


def same_group_pairs(groups):
    """Every pair i < j with groups[i] == groups[j], by (i, j) ascending: two int64 arrays."""
    g = np.asarray(groups).reshape(-1)
    n = len(g)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    order = np.argsort(g, kind="stable").astype(np.int64)          # by group, ascending index inside a group
    sg = g[order]
    lead = np.concatenate([[True], sg[1:] != sg[:-1]])
    end = np.append(np.flatnonzero(lead)[1:], n)[np.cumsum(lead) - 1]         # one past the last place of its group
    count = end - np.arange(n) - 1                                  # partners behind each place
    place = np.repeat(np.arange(n), count)
    within = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
    first, second = order[place], order[place + 1 + within]
    by = np.lexsort((second, first))
    return first[by], second[by]


def csr_of_pairs(n, first, second, ed):
    """The hit list of listed pairs (first < second, sorted by (first, second)) and their distances: those not -1."""
    keep = np.asarray(ed) != -1
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(first[keep], minlength=n), out=off[1:])
    return {"rowOffsets": off, "partner": second[keep].astype(np.int32), "editDistance": np.asarray(ed)[keep].astype(np.int32)}


def interleaved_labels(sizes=SIZES, labels=LABELS):
    """member x of every group in turn: no group is contiguous"""
    out = []
    for x in range(max(sizes)):
        out += [lab for size, lab in zip(sizes, labels) if x < size]
    return np.array(out, dtype=np.int64)


def _rand(rng, m):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(m))].tobytes()


def _mutate(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        at = int(rng.integers(0, len(s)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            s[at] = b"ACGT"[int(rng.integers(0, 4))]
        elif kind == 1:
            s.insert(at, b"ACGT"[int(rng.integers(0, 4))])
        elif len(s) > 20:
            del s[at]
    return bytes(s)


def planted_set(seed=5):
    """222 sequences of 20..40 bases over ACGT in groups of the sizes above, labels interleaved.  Every group has a few
    founders and mutated copies (0..3 edits), so hits occur at k = 0, 2 and 5.  Planted: one sequence copied into five
    different groups (never a hit), and one copied twice more inside the group of 65 (distance-0 hits).
    Returns (seqs, groups, planted) with planted = {"across": indices, "inside": indices}."""
    rng = np.random.default_rng(seed)
    groups = interleaved_labels()
    seqs = [None] * len(groups)
    for part in members_of(groups).values():
        founders = [_rand(rng, rng.integers(20, 41)) for _ in range(1 + len(part) // 16)]
        for i in part:
            seqs[int(i)] = _mutate(rng, founders[int(rng.integers(0, len(founders)))], int(rng.integers(0, 4)))
    mem = members_of(groups)
    across = [int(mem[lab][-1]) for lab in (LABELS[3], LABELS[4], LABELS[6], LABELS[7], LABELS[8])]
    for i in across:
        seqs[i] = seqs[across[0]]
    inside = [int(x) for x in mem[LABELS[8]][[0, 20, 40]]]
    for i in inside:
        seqs[i] = seqs[inside[0]]
    return seqs, groups, {"across": across, "inside": inside}


def big_group_case(seed=6):
    """One group of 1,500 among 500 singletons, 28..32 bases, a third of the group near one founder."""
    rng = np.random.default_rng(seed)
    groups = np.array([100 + i if i % 4 == 3 else 7 for i in range(2000)], dtype=np.int64)
    founder = _rand(rng, 30)
    seqs = [_mutate(rng, founder, int(rng.integers(0, 3))) if rng.random() < 0.34 else _rand(rng, rng.integers(28, 33))
            for _ in range(2000)]
    return seqs, groups


def scattered_case(seed=8):
    """300 sequences of 20..40 bases in ten groups, and in the groups 0, 4 and 9 a 200-base sequence with a relative of
    201 bases each, at scattered positions: the seven-word group's tile spans distant ranks."""
    rng = np.random.default_rng(seed)
    seqs = [_rand(rng, rng.integers(20, 41)) for _ in range(300)]
    groups = [i % 10 for i in range(300)]
    for g in (0, 4, 9):
        long = _rand(rng, 200)
        at = int(rng.integers(0, len(seqs)))
        seqs.insert(at, long)
        groups.insert(at, g)
        seqs.append(long[:77] + b"A" + long[77:])
        groups.append(g)
    return seqs, np.array(groups, dtype=np.int64)
