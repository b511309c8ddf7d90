"""No GPU: (1) the pairs of flat_cigar_cases.py reach the edges of the device's CIGAR kernel -- asserted on the
reference's own strings, so that test_gpu_flat_cigar_cases.py is known to aim where it says; (2) this library's host
edlibAlignmentToCigar against the checker's over random op strings: it is the yardstick of
test_batch_cigars_equal_edlibAlignmentToCigar and had one 11-op known answer of its own."""
import re

import numpy as np
import pytest

import edlib_amd
import flat_cigar_cases as cases
from oracle import oracle as O

_RUN = re.compile(r"(\d+)([=XIDM])")


def _strings(ref, extended):
    off = ref["cigExtOff" if extended else "cigStdOff"]
    raw = ref["cigExt" if extended else "cigStd"]
    return [raw[int(off[u]):int(off[u + 1])].decode() for u in range(len(off) - 1)]


def _runs(s):
    """[(first op index, length, letter)] of a CIGAR string"""
    out, at = [], 0
    for n, c in _RUN.findall(s):
        out.append((at, int(n), c)); at += int(n)
    assert "".join("%d%s" % (n, c) for _, n, c in out) == s
    return out


@pytest.fixture(scope="module")
def nw_ref():
    qs, ts, what = cases.nw_pairs()
    qoff = np.zeros(len(qs) + 1, dtype=np.int64); qoff[1:] = np.cumsum([len(q) for q in qs])
    toff = np.zeros(len(ts) + 1, dtype=np.int64); toff[1:] = np.cumsum([len(t) for t in ts])
    return O.pool_align(np.concatenate(qs), qoff, np.concatenate(ts), toff, False, "NW", "path", -1, want_cigar=True)


def test_the_list_is_a_flat_batch():
    qs, ts, what = cases.nw_pairs()
    assert len(qs) == len(ts) == len(what) >= cases.MIN_UNITS >= 1024
    assert all(1 <= len(q) <= 1024 and 1 <= len(t) <= 1024 for q, t in zip(qs, ts))
    assert set(np.unique(np.concatenate(qs + ts)).tolist()) <= set(b"ACGT")
    qs, ts, what = cases.window_pairs()
    assert len(qs) == len(ts) == len(what) >= cases.MIN_UNITS
    assert all(1 <= len(q) <= 256 for q in qs)            # (SHW / HW paths stay flat up to 4 blocks)


def test_no_unit_leaves_the_flat_path(nw_ref):
    """without a threshold every unit is inside the first band level: the run stays flat, the CIGARs are the device's"""
    qs, ts, what = cases.nw_pairs()
    out = [(u, what[u], int(d)) for u, d in enumerate(nw_ref["editDistance"]) if len(qs[u]) > cases.WHOLE_RING and d > cases.FIRST_LEVEL]
    assert not out, out[:5]
    assert sum(len(q) > cases.WHOLE_RING for q in qs) > 300


def test_the_planted_pairs_align_as_planted(nw_ref):
    qs, ts, what = cases.nw_pairs()
    ext, std = _strings(nw_ref, True), _strings(nw_ref, False)
    at = {w: u for u, w in enumerate(what)}
    for L in cases.IDENTICAL:
        assert ext[at["identical %d" % L]] == "%d=" % L and std[at["identical %d" % L]] == "%dM" % L
        u = at["identical %d, substitution at %d" % (L, L - 1)]
        assert ext[u] == ("%d=" % (L - 1) if L > 1 else "") + "1X" and std[u] == "%dM" % L
    for L in cases.ALTERNATING:
        u = at["alternating %d" % L]
        want = "1=1X" * (L // 2) + "1=" * (L & 1) if L <= cases.WHOLE_RING else "65=1X" + "1=1X" * 119 + "%d=" % (L - 304)
        assert ext[u] == want and std[u] == "%dM" % L


def test_extended_strings_reach_the_edges_of_the_run_logic(nw_ref):
    runs = [_runs(s) for s in _strings(nw_ref, True)]
    lengths = {n for r in runs for _, n, _ in r}
    assert {9, 10, 99, 100, 999, 1000} <= lengths                      # dec_digits at every width a flat batch has
    starts = {at % 64 for r in runs for at, _, _ in r if at > 0}
    assert {0, 1, 63} <= starts                                        # a run closed by lane 0, 1 and 63 of a trip
    assert any(n > 128 and at + n > (at // 64 + 2) * 64 for r in runs for at, n, _ in r)   # a run open across whole trips
    # 64 closes in one trip: every op of an aligned span of 64 starts a run, and the span is not the string's first
    # (op 0 starts a run but closes none)
    full = False
    for r in runs:
        first = np.array([at for at, _, _ in r], dtype=np.int64)
        per_span = np.bincount(first // 64)
        full = full or bool((per_span[1:] == 64).any())
    assert full


def test_standard_runs_cover_a_class_change_at_a_trip_edge(nw_ref):
    """an '=' next to an 'X' with the second at an op index that is a multiple of 64: the class carried into the trip
    (prevCls) has to be the merged one, or the standard-format M run is cut there"""
    hit = 0
    for e, s in zip(_strings(nw_ref, True), _strings(nw_ref, False)):
        ops = "".join(c * n for _, n, c in _runs(e))
        std = "".join(c * n for _, n, c in _runs(s))
        assert len(ops) == len(std)
        covered = {at + j for at, n, c in _runs(s) if c == "M" for j in range(1, n)}   # indices inside an M run, not its first
        for i in range(64, len(ops), 64):
            if {ops[i - 1], ops[i]} == {"=", "X"}:
                assert i in covered
                hit += 1
    assert hit >= 10


@pytest.mark.parametrize("mode", ["HW", "SHW"])
def test_all_mismatching_queries_are_m_inserts(mode):
    qs, ts, what = cases.window_pairs()
    qoff = np.zeros(len(qs) + 1, dtype=np.int64); qoff[1:] = np.cumsum([len(q) for q in qs])
    toff = np.zeros(len(ts) + 1, dtype=np.int64); toff[1:] = np.cumsum([len(t) for t in ts])
    ref = O.pool_align(np.concatenate(qs), qoff, np.concatenate(ts), toff, False, mode, "path", -1, want_cigar=True)
    ext = _strings(ref, True)
    seen = set()
    for u, w in enumerate(what):
        if "mismatches" in w:
            m = len(qs[u])
            assert ext[u] == "%dI" % m and ref["ends"][ref["locOff"][u]] == -1 and ref["numLocations"][u] <= 16, (u, w)
            seen.add(m)
    assert seen == set(cases.LEAD_INSERTS)
    assert ref["numLocations"].max() <= 16                             # nobody sends the batch to the general path


# ---------------------------------------------------------------- the host edlibAlignmentToCigar

_EDGE_RUNS = (1, 2, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, 9999, 10000, 10001)
_LONG_RUNS = (99999, 100000, 100001, 999999, 1000000)


def _op_strings():
    rng = np.random.default_rng(77)
    out = [b""]
    for i in range(300):
        nruns = int(rng.integers(1, 40))
        ops = rng.integers(0, 4, nruns)                                # (neighbours may repeat, 0 and 3 merge in the standard form)
        lens = np.where(rng.random(nruns) < 0.3, rng.choice(_EDGE_RUNS, nruns), rng.integers(1, 13, nruns))
        if i % 20 == 0:                                                # 5- to 7-digit lengths: 10^4 .. 10^6 ops in a run
            lens[int(rng.integers(nruns))] = int(10 ** rng.uniform(4, 6))
            lens[int(rng.integers(nruns))] = int(rng.choice(_LONG_RUNS))
        out.append(np.repeat(ops.astype(np.uint8), lens).tobytes())
    for n in _LONG_RUNS:                                               # a single run (the last one is closed behind the loop)
        out.append(bytes([int(rng.integers(0, 4))]) * n)
    return out


def test_host_cigar_equals_the_checker(checker):
    digits = set()
    for ops in _op_strings():
        for extended in (True, False):
            want = checker.cigar(ops, 1 if extended else 0)
            got = edlib_amd.cigar_from_alignment(ops, extended)
            assert want is not None and got == want, (len(ops), extended, got[:60] if got else got, want[:60])
            digits |= {len(n) for n, _ in _RUN.findall(want)}
    assert {1, 2, 3, 4, 5, 6, 7} <= digits
    assert edlib_amd.cigar_from_alignment(b"", True) == "" and edlib_amd.cigar_from_alignment(b"", False) == ""


@pytest.mark.parametrize("bad", [b"\x00\x04", b"\x00\x00\x07\x01", b"\x01\x02\xff", b"\x04", b"\x04\x00"])
def test_host_cigar_refuses_an_invalid_op(checker, bad):
    """NULL.  The reference looks an op up in its table of four letters BEFORE it tests the code, and tests it only where
    a run closes (edlib.cpp:311-341): an invalid code behind a valid op is refused, a leading one is read past the table.
    The checker is asked where the reference's answer is defined; this library refuses both."""
    for extended in (True, False):
        if bad[0] <= 3:
            assert checker.cigar(bad, 1 if extended else 0) is None
        assert edlib_amd.cigar_from_alignment(bad, extended) is None
