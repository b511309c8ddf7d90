"""Pairs whose paths reach the edges of the device's CIGAR kernel (flat_results.hip: cigar_kernel -- a wave per op
string, 64 ops per trip, runs closed by a ballot, the open run and the last class carried across trips, '=' and 'X'
merged in the standard format, run lengths sized by dec_digits).  test_flat_cigar_cases.py asserts on the reference's
strings alone that these inputs get there; test_gpu_flat_cigar_cases.py runs them through flat pair batches.  A plain
module, not a conftest."""
import functools

import numpy as np

from edlib_amd import synth

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_AC = np.frombuffer(b"AC", dtype=np.uint8)
_GT = np.frombuffer(b"GT", dtype=np.uint8)

IDENTICAL = (1, 9, 10, 63, 64, 65, 99, 100, 127, 128, 129, 999, 1000, 1023, 1024)
SUBSTITUTED_AT = (0, 62, 63, 64, 65, 127, 128)            # and L - 1
ALTERNATING = (64, 65, 128, 200, 1000)
GAPS = (9, 10, 63, 64, 65, 99, 100)
GAP_TARGETS = (300, 1000)
LEAD_INSERTS = (9, 10, 63, 65, 99, 100, 127, 129)         # no multiple of 64: the empty prefix comes first
MIN_UNITS = 1100                                          # (a flat batch has at least 1,024)
# An NW PATH batch stays on the flat path -- and its CIGARs are made on the device -- while no unit fails the first band
# level (flat_pairs_prepare.hpp: flat_desc): a query of up to 8 words of 32 rows sits whole on its ring, a longer one
# has the band of K = 128.  One unit beyond it sends the whole run to the general path, whose CIGARs the host makes.
WHOLE_RING, FIRST_LEVEL = 256, 128


def _other(b):
    return _ACGT[(int(np.searchsorted(_ACGT, b)) + 1) % 4]


@functools.lru_cache(maxsize=None)
def nw_pairs():
    """(queries, targets, what): `what[u]` names the case of unit u"""
    rng = np.random.default_rng(1303)
    qs, ts, what = [], [], []

    def add(q, t, name):
        qs.append(np.ascontiguousarray(q[:1024])); ts.append(np.ascontiguousarray(t)); what.append(name)

    for L in IDENTICAL:                                    # one run of L: L= / LM
        t = _ACGT[rng.integers(0, 4, L)]
        add(t.copy(), t, "identical %d" % L)
        for p in sorted(set(SUBSTITUTED_AT + (L - 1,))):   # p= 1X (L-p-1)=, one LM whose class changes at p and p + 1
            if p < L:
                q = t.copy(); q[p] = _other(t[p])
                add(q, t, "identical %d, substitution at %d" % (L, p))
    for L in ALTERNATING:                                  # 1=1X1=1X...: every op closes a run; one LM
        t = _AC[rng.integers(0, 2, L)]
        q = t.copy()
        # (a query above 256 bases has to stay within FIRST_LEVEL: ops 64 .. 303 alternate, 120 substitutions)
        odd = slice(1, None, 2) if L <= WHOLE_RING else slice(65, 304, 2)
        q[odd] = _GT[rng.integers(0, 2, len(q[odd]))]
        add(q, t, "alternating %d" % L)
    for T in GAP_TARGETS:                                  # blocks of g inserted into / deleted from the query
        for g in GAPS:
            for at in (54, 55, 64, 128 - g):
                t = _ACGT[rng.integers(0, 4, min(T, 1024 - g))]   # (the query is not cut: the block is the whole distance)
                add(np.concatenate([t[:at], _ACGT[rng.integers(0, 4, g)], t[at:]]), t, "target %d, %d inserted at %d" % (T, g, at))
                t = _ACGT[rng.integers(0, 4, T)]
                add(np.concatenate([t[:at], t[at + g:]]), t, "target %d, %d deleted at %d" % (T, g, at))
    rates = ((0.03, 0.01), (0.2, 0.1), (0.0, 0.0))
    while len(qs) < MIN_UNITS:                             # ordinary mutated pairs up to the flat threshold
        sub, indel = rates[len(qs) % len(rates)]
        T = int(rng.choice((5, 64, 150, 700, 1000) if sub < 0.1 else (5, 64, 150)))
        t = _ACGT[rng.integers(0, 4, T)]
        q, _ = synth.mutate(t, int(rng.integers(1 << 30)), sub, indel, indel)
        add(q if len(q) else _ACGT[:1].copy(), t, "mutated %d" % T)
    return qs, ts, what


@functools.lru_cache(maxsize=None)
def window_pairs():
    """SHW / HW: reads of 150 bases in windows of 400 and, among them, queries that match nothing of their target: the
    empty prefix is the first location and the path is m inserts"""
    rng = np.random.default_rng(1304)
    qs, ts, what = [], [], []
    for i in range(MIN_UNITS):
        t = _ACGT[rng.integers(0, 4, 400)]
        a = int(rng.integers(0, 9))                        # (near the window's first column: SHW sees the read too)
        q, _ = synth.mutate(t[a:a + 150], int(rng.integers(1 << 30)), 0.03, 0.01, 0.01)
        qs.append(np.ascontiguousarray(q)); ts.append(t); what.append("150 in 400")
    at = 3
    for T in (1, 7, 15):                                   # (at most 16 end locations: the unit keeps its flat list)
        for m in LEAD_INSERTS:
            qs[at] = np.full(m, ord("A"), dtype=np.uint8); ts[at] = np.full(T, ord("C"), dtype=np.uint8)
            what[at] = "%d mismatches, target %d" % (m, T)
            at += 41
    return qs, ts, what
