"""GPU: window units with a strand (edlibAmdBatchCreateWindowsStranded).  A strand-1 unit is reverse_complement(query) against
its window: the expected units come from the checker (the compiled reference where it travelled) on the sliced window with
that query, best() from window_best_model() over all units of a query whatever their strand."""
import numpy as np
import pytest

import edlib_amd
from edlib_amd import reverse_complement, synth, window_best_model
from test_gpu_windows import FIELDS, IUPAC, _bytes, _read_from, host_word_steps, ref_units

pytestmark = pytest.mark.gpu


def ref_stranded(queries, target, uq, us, ul, strand, mode, k, eqs=None):
    """The checker over the expanded query list [q0, rc(q0), q1, rc(q1), ...] with unit u naming entry 2 q + strand."""
    both = []
    for q in queries:
        both += [_bytes(q), reverse_complement(_bytes(q))]
    return ref_units(both, target, [2 * int(q) + int(s) for q, s in zip(uq, strand)], us, ul, mode, k, eqs)


def check(b, queries, target, uq, us, ul, strand, mode, k, eqs=None):
    got = b.units()
    want = ref_stranded(queries, target, uq, us, ul, strand, mode, k, eqs)
    for f in FIELDS:
        assert got[f].shape == (len(uq),) and got[f].dtype == np.int32, f
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, mode, k, [(int(i), int(got[f][i]), int(want[f][i]), len(queries[int(uq[i])]),
                                             int(strand[i]), int(us[i]), int(ul[i])) for i in bad[:5]])
    best = b.best()
    model = window_best_model(uq, got["editDistance"], len(queries))
    for f, v in model.items():
        assert best[f].dtype == np.int32 and np.array_equal(best[f], v), (f, np.nonzero(best[f] != v)[0][:5])
    assert b.stats()["cells"] == sum(len(queries[int(q)]) * int(n) for q, n in zip(uq, ul))
    return got, best


def _plant(target, pos, seq):
    target[pos:pos + len(seq)] = np.frombuffer(seq, dtype=np.uint8)


# ---- 1. mixed strands

@pytest.mark.parametrize("mode,k", [("HW", -1), ("HW", 6), ("NW", 40), ("SHW", 12)])
def test_mixed_strands(engine, checker, mode, k):
    rng = np.random.default_rng(11)
    target = np.array(synth.random_dna(301, 20_000), dtype=np.uint8)
    lens = [20, 31, 32, 33, 64, 65, 100, 128, 129, 140, 150, 150]
    queries, loci = [], []
    for i, m in enumerate(lens):
        pos = 500 + 1500 * i
        q = _read_from(target, pos, m, rng, 2)
        queries.append(q)
        _plant(target, pos + 700, reverse_complement(q))        # a locus that holds the reverse complement
        loci.append((pos, pos + 700))
    uq, us, ul, strand = [], [], [], []
    for u in range(130):
        q = u % 12
        s = int(rng.integers(0, 2)) if u >= 24 else u // 12       # every query is named on both strands
        fwd_locus, rev_locus = loci[q]
        at = (rev_locus if (u // 12) % 2 == 0 else fwd_locus) if s else (fwd_locus if (u // 12) % 3 else int(rng.integers(0, 19_000)))
        pad = int(rng.integers(0, 30 if mode == "HW" else 3))
        start = max(0, at - pad)
        uq.append(q); us.append(start); ul.append(min(len(queries[q]) + 2 * pad, 20_000 - start))
        strand.append(s)
    assert all({(q, 0), (q, 1)} <= set(zip(uq, strand)) for q in range(12))
    b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k, unit_strand=strand)
    try:
        st = b.run()
        assert st["path"] & 16 and not st["path"] & 2, st
        got, best = check(b, queries, target, uq, us, ul, strand, mode, k)
        assert st["word_steps"] == host_word_steps(queries, uq, ul, mode, k), st
        rev_hits = [u for u in range(130) if strand[u] and got["editDistance"][u] >= 0 and got["editDistance"][u] <= 4]
        assert rev_hits, "no strand-1 unit found its planted reverse complement"
        assert any(strand[int(u)] for u in best["bestUnit"] if u >= 0)
    finally:
        b.close()


# ---- 2. the same locus on both strands

def test_same_locus_both_strands(engine, checker):
    rng = np.random.default_rng(12)
    target = np.array(synth.random_dna(302, 3000), dtype=np.uint8)
    q = _read_from(target, 400, 60, rng, 0)
    _plant(target, 1500, reverse_complement(q))
    half = _read_from(target, 2000, 15, rng, 0)
    pal = half + reverse_complement(half)
    _plant(target, 2500, pal)
    queries = [q, pal]
    for locus, planted in ((380, 0), (1480, 1)):
        uq, us, ul, strand = [0, 0, 1, 1], [locus, locus, 2480, 2480], [100, 100, 70, 70], [0, 1, 1, 0]
        b = engine.WindowBatch(queries, target, uq, us, ul, mode="HW", k=-1, unit_strand=strand)
        try:
            b.run()
            got, best = check(b, queries, target, uq, us, ul, strand, "HW", -1)
            assert best["bestUnit"][0] == planted and best["bestDistance"][0] == 0       # the planted strand wins
            assert best["secondDistance"][0] == got["editDistance"][1 - planted] > 0      # the other strand is second
            assert got["editDistance"][2] == got["editDistance"][3] == 0                   # a palindrome ties:
            assert best["bestUnit"][1] == 2 and best["secondDistance"][1] == 0             # the lower unit index
        finally:
            b.close()


# ---- 3. a NULL unitStrand is a plain window batch

def test_null_unit_strand_equals_plain(engine):
    import ctypes as C
    rng = np.random.default_rng(13)
    target = np.array(synth.random_dna(303, 5000), dtype=np.uint8)
    queries = [_read_from(target, int(p), int(m), rng, 2) for p, m in ((100, 30), (900, 64), (2000, 150))]
    uq = rng.integers(0, 3, size=50).astype(np.int32)
    us = rng.integers(0, 4500, size=50).astype(np.int32)
    ul = rng.integers(0, 400, size=50).astype(np.int32)
    L = engine.lib()
    qd, qo = engine._pack(queries)
    cfg, keep = engine._make_config("HW", "distance", 5, None)
    h = L.edlibAmdBatchCreateWindowsStranded(qd.ctypes.data, qo.ctypes.data, 3, target.ctypes.data, len(target),
                                             uq.ctypes.data, us.ctypes.data, ul.ctypes.data, None, 50, cfg, 0)
    assert h, engine.last_error()
    try:
        assert L.edlibAmdBatchRun(h) == 0
        v = engine.WindowView()
        assert L.edlibAmdBatchWindowView(h, 3, C.byref(v)) == 0
        null = {f: np.ctypeslib.as_array(getattr(v, f), shape=(50,)).copy() for f in FIELDS}
        null.update({f: np.ctypeslib.as_array(getattr(v, f), shape=(3,)).copy()
                     for f in ("bestUnit", "bestDistance", "secondDistance")})
    finally:
        L.edlibAmdBatchDestroy(h)
    plain = engine.align_windows(queries, target, uq, us, ul, mode="HW", k=5)
    zeros = engine.align_windows(queries, target, uq, us, ul, mode="HW", k=5, unit_strand=np.zeros(50, dtype=np.uint8))
    assert len(plain) == 6
    for f in plain:
        assert np.array_equal(null[f], plain[f]), f
        assert np.array_equal(zeros[f], plain[f]), f


# ---- 4. outside the kernel's envelope: the pair route reverse-complements on the host

@pytest.mark.parametrize("mode,k", [("HW", 10), ("NW", 10)])
def test_envelope(engine, checker, mode, k):
    rng = np.random.default_rng(14)
    target = np.array(synth.random_dna(304, 6000), dtype=np.uint8)
    long_q = _read_from(target, 1000, 300, rng, 3)
    _plant(target, 3000, reverse_complement(long_q))
    short = _read_from(target, 200, 80, rng, 1)
    _plant(target, 5000, reverse_complement(short))
    queries = [long_q, short]
    pad = 0 if mode == "NW" else 20
    uq = [0, 0, 0, 0, 1, 1, 1]
    us = [1000 - pad, 3000 - pad, 3000 - pad, 1000 - pad, 200 - pad, 5000 - pad, 5000 - pad]
    ul = [300 + 2 * pad] * 4 + [80 + 2 * pad] * 3
    strand = [0, 1, 0, 1, 0, 1, 0]
    b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k, unit_strand=strand)
    try:
        st = b.run()
        assert st["path"] & 16 and st["path"] & 2, st
        got, best = check(b, queries, target, uq, us, ul, strand, mode, k)
        assert 0 <= got["editDistance"][1] <= 3 and got["editDistance"][2] == -1      # the long query's reverse complement
        assert 0 <= got["editDistance"][5] <= 1 and got["editDistance"][6] == -1
        assert best["bestUnit"].tolist() == [0 if got["editDistance"][0] <= got["editDistance"][1] else 1,
                                             4 if got["editDistance"][4] <= got["editDistance"][5] else 5]
    finally:
        b.close()


# ---- 5. word-count boundaries on strand 1, IUPAC with equalities

def test_word_count_boundaries(engine, checker):
    rng = np.random.default_rng(15)
    target = np.array(synth.random_dna(305, 6000), dtype=np.uint8)
    at = rng.integers(0, 6000, size=300)
    target[at] = rng.choice(np.frombuffer(b"RYN", dtype=np.uint8), size=300)
    queries, uq, us, ul, strand = [], [], [], [], []
    for i, m in enumerate((32, 33, 256)):
        pos = 300 + 1500 * i
        q = bytearray(_read_from(target, pos, m, rng, 1))
        q[m // 2] = ord("R")
        q = bytes(q)
        queries.append(q)
        _plant(target, pos + 600, reverse_complement(q))
        for start, n, s in ((pos + 590, m + 20, 1), (pos + 590, m + 20, 0), (pos - 10, m + 20, 0), (pos - 10, m + 20, 1),
                            (pos + 600, m, 1)):
            uq.append(i); us.append(start); ul.append(n); strand.append(s)
    for mode, k in (("HW", -1), ("HW", 3), ("NW", 25), ("SHW", 30)):
        b = engine.WindowBatch(queries, target, uq, us, ul, mode=mode, k=k, additionalEqualities=IUPAC, unit_strand=strand)
        try:
            st = b.run()
            assert st["path"] & 16 and not st["path"] & 2, st
            got, best = check(b, queries, target, uq, us, ul, strand, mode, k, IUPAC)
            if mode == "HW":
                assert all(got["editDistance"][5 * i] == 0 for i in range(3))         # strand 1 on the planted locus
                assert all(strand[int(u)] == 1 or got["editDistance"][int(u)] == 0 for u in best["bestUnit"])
        finally:
            b.close()
