"""CPU: the model side of both-strand read batches (tests/strand_cases.py) -- the complement table and the
host-only edlibAmdReverseComplement, the rule that picks a strand against the oracle on small cases, the failure behaviour
of the two new batch entry points without a device, and the preconditions every batch of tests/test_gpu_strands.py relies
on, checked with tests/seed_model.py."""
import ctypes as C

import numpy as np
import pytest

import seed_model as SM
import strand_cases as SC
from oracle.oracle import load_oracle


def _nslots(n):
    return (n + 63) // 64 * 64


def test_complement_table():
    c = SC.COMP
    codes = [b for b in SC.CODES if chr(b) not in "Uu"]
    for b in codes:
        assert c[c[b]] == b, chr(b)                               # an involution on the nucleotide codes ...
    assert c[ord("U")] == ord("A") and c[ord("u")] == ord("a") and c[ord("A")] == ord("T")    # ... except U
    for b in b"SWNswn":
        assert c[b] == b
    for a, b in (("A", "T"), ("C", "G"), ("R", "Y"), ("K", "M"), ("B", "V"), ("D", "H")):
        assert c[ord(a)] == ord(b) and c[ord(a.lower())] == ord(b.lower())
    rest = [b for b in range(256) if b not in SC.CODES]
    assert all(c[b] == b for b in rest)                           # identity everywhere else
    assert bytes(SC.rc(b"AACGTN")) == b"NACGTT" and bytes(SC.rc(b"")) == b""


@pytest.mark.parametrize("n", [0, 1, 255, 4097])
def test_reverse_complement_entry_point(n):
    """edlibAmdReverseComplement through ctypes equals numpy on random bytes 0..255 (host only: no device needed)"""
    import edlib_amd
    L = edlib_amd.lib()
    src = np.random.default_rng(n).integers(0, 256, n).astype(np.uint8)
    out = np.full(n + 2, 0xAB, dtype=np.uint8)
    L.edlibAmdReverseComplement(src.ctypes.data if n else None, n, out.ctypes.data)
    assert np.array_equal(out[:n], SC.rc(src)) and out[n] == 0xAB
    assert edlib_amd.reverse_complement(src.tobytes()) == SC.rc(src).tobytes()
    assert np.array_equal(edlib_amd.reverse_complement(src), SC.rc(src))


def test_resolve_covers_the_table():
    orc = load_oracle()
    seen = set()
    for name, q, t, mode, k in SC.table_rows():
        rp = orc.align(q, t, mode, "path", k)
        rm = orc.align(bytes(SC.rc(q)), t, mode, "path", k)
        got, strand, both = SC.resolve(rp, rm)
        dp, dm = rp["editDistance"], rm["editDistance"]
        s2, b2 = SC.strands_of(np.array([dp, dm]))
        assert (int(s2[0]), int(b2[0])) == (strand, both), name
        if name.startswith("forward only"):
            assert dp >= 0 and dm < 0 and (strand, both) == (0, 0) and got is rp
        if name.startswith("reverse only"):
            assert dp < 0 and dm >= 0 and (strand, both) == (1, 0) and got is rm
        if name.startswith("forward better"):
            assert 0 <= dp < dm and (strand, both) == (0, 0)
        if name.startswith("reverse better"):
            assert 0 <= dm < dp and (strand, both) == (1, 0) and got is rm
        if name.startswith("neither"):
            assert dp == dm == -1 and (strand, both) == (0, 0) and got is rp
        if name in ("palindrome", "empty read", "tie of two different strands"):
            assert dp == dm >= 0 and (strand, both) == (0, 1) and got is rp
        seen.add((strand, both, dp >= 0, dm >= 0))
    assert {(0, 0, True, False), (1, 0, False, True), (0, 0, False, False), (0, 1, True, True), (1, 0, True, True),
            (0, 0, True, True)} <= seen


def test_resolve_flat_is_resolve_per_read():
    """the numpy statement over a flat 2n-unit result picks, field by field, what resolve() picks per read"""
    orc = load_oracle()
    rows = SC.table_rows()[:8]
    t = rows[0][2]
    reads = [np.frombuffer(q, dtype=np.uint8) for _, q, tt, _, _ in rows if tt == t]
    per, d2, ends, starts, aln, alpha = [], [], [], [], [], []
    for s in SC.interleave(reads):
        r = orc.align(s.tobytes(), t, "HW", "path", -1)
        per.append(r)
        d2.append(r["editDistance"]); ends.append(r["endLocations"] or [])
        starts.append(r["startLocations"] if r["startLocations"] is not None else [-1] * len(ends[-1]))   # (an empty read has none)
        aln.append(r["alignment"] or b""); alpha.append(r["alphabetLength"])
    lo = np.zeros(len(per) + 1, dtype=np.int64); lo[1:] = np.cumsum([len(e) for e in ends])
    ao = np.zeros(len(per) + 1, dtype=np.int64); ao[1:] = np.cumsum([len(a) for a in aln])
    flat = {"status": np.zeros(len(per), dtype=np.int32), "editDistance": np.array(d2, dtype=np.int32),
            "numLocations": np.array([len(e) for e in ends], dtype=np.int32), "alphabetLength": np.array(alpha, dtype=np.int32),
            "locOff": lo, "ends": np.array([x for e in ends for x in e], dtype=np.int32),
            "starts": np.array([x for e in starts for x in e], dtype=np.int32),
            "alnOff": ao, "alignment": np.frombuffer(b"".join(aln), dtype=np.uint8)}
    got = SC.resolve_flat(flat, "path")
    for i in range(len(reads)):
        want, strand, both = SC.resolve(per[2 * i], per[2 * i + 1])
        assert (got["strand"][i], got["bothStrands"][i]) == (strand, both)
        assert got["editDistance"][i] == want["editDistance"] and got["alphabetLength"][i] == want["alphabetLength"]
        a, b = got["locOff"][i], got["locOff"][i + 1]
        assert list(got["ends"][a:b]) == list(want["endLocations"] or []) and list(got["starts"][a:b]) == list(want["startLocations"] or [-1] * int(b - a))
        a, b = got["alnOff"][i], got["alnOff"][i + 1]
        assert bytes(got["alignment"][a:b]) == (want["alignment"] or b"")


def test_new_entry_points_fail_cleanly_without_a_device():
    import edlib_amd
    L = edlib_amd.lib()
    sv = edlib_amd.StrandView()
    assert L.edlibAmdBatchStrandView(None, C.byref(sv)) == 1 and "null" in edlib_amd.last_error()
    if edlib_amd.device_count() > 0:
        return                                                    # (creation on a device: tests/test_gpu_strands.py)
    cfg = L.edlibDefaultAlignConfig()
    q = np.frombuffer(b"ACGTACGT", dtype=np.uint8).copy()
    off = np.array([0, 4, 8], dtype=np.int64)
    t = np.frombuffer(b"ACGTTTACGT", dtype=np.uint8).copy()
    h = L.edlibAmdBatchCreateSharedBothStrands(q.ctypes.data, off.ctypes.data, 2, t.ctypes.data, len(t), cfg, 0)
    assert not h and "no CPU fallback" in edlib_amd.last_error()
    with pytest.raises(RuntimeError):
        edlib_amd.BothStrandsBatch([b"ACGT"], b"ACGTACGT")
    with pytest.raises(RuntimeError):
        edlib_amd.align_batch([b"ACGT"], b"ACGTACGT", strands="both")
    with pytest.raises(ValueError):
        edlib_amd.align_batch([b"ACGT"], b"ACGTACGT", strands="reverse")


# ------------------------------------------------------------------- preconditions of the GPU batches (test_gpu_strands.py)

@pytest.mark.parametrize("nwd", [5, 8])
def test_seed_only_batches_meet_their_preconditions(nwd):
    """test 2: fewer than 16,384 slots, slots x T >= 2^30, at most 1 % of the reads dropped, the model hands nothing back on
    either strand, every kept read resolves at k_f on at least one strand, the wrong strands add little"""
    b = SC.seeded_group(nwd)
    T, kf = len(b["target"]), b["kf"]
    both = SC.interleave(b["reads"])
    slots = _nslots(len(both))
    assert slots < 16_384 and slots * T >= 1 << 30
    assert 0 < len(b["reads"]) and b["dropped"] * 100 <= 2_230
    assert all((len(r) + 31) // 32 == nwd for r in b["reads"])
    assert kf == SM.seed_threshold(min(len(r) for r in b["reads"]), T) >= 8
    pred = SM.predict_batch(both, b["target"], kf)
    assert sum(p["back"] for p in pred) == 0
    cols = np.array([p["columns"] for p in pred])
    assert cols.sum() > 0 and nwd * cols.sum() * 1000 < slots * T * nwd          # far below one word per column per slot
    print("nwd=%d: %d reads kept, %d dropped, columns %d" % (nwd, len(b["reads"]), b["dropped"], int(cols.sum())))


@pytest.mark.parametrize("nwd", [5, 8])
def test_climbing_batches_meet_their_preconditions(nwd):
    """tests 3 and 6: fewer than 16,384 slots (no ladder is priced), the seed pass is eligible, reads of one word count"""
    b = SC.seeded_group(nwd, only_resolving=False)
    slots = _nslots(2 * len(b["reads"]))
    assert 1_024 <= slots < 16_384 and slots * len(b["target"]) >= 1 << 30 and len(b["target"]) >= 64 * 32 * nwd
    assert all((len(r) + 31) // 32 == nwd for r in b["reads"])
    assert b["kf"] == SM.seed_threshold(min(len(r) for r in b["reads"]), len(b["target"])) >= 8


@pytest.mark.parametrize("kind", ["three", "five_n"])
def test_banded_batches_meet_their_preconditions(kind):
    """test 4: no seed pass (k_f below 8 on four symbols; five symbols), fewer than 16,384 slots"""
    b = SC.banded_group(kind)
    nwd = b["nwd"]
    assert all((len(r) + 31) // 32 == nwd for r in b["reads"]) and _nslots(2 * len(b["reads"])) < 16_384
    sigma = len(set(b["target"].tolist()))
    if kind == "three":
        assert sigma == 4 and SM.seed_threshold(min(len(r) for r in b["reads"]), len(b["target"])) < 8
    else:
        assert sigma == 5


def test_view_batch_meets_its_preconditions():
    """test 5: two word groups, at least 1,025 slots each"""
    b = SC.two_groups()
    words = {}
    for r in b["reads"]:
        words[(len(r) + 31) // 32] = words.get((len(r) + 31) // 32, 0) + 2
    assert len(words) == 2 and all(_nslots(v) >= 1_025 for v in words.values())


def test_parity_batches_cover_every_route():
    """test 1: all eight word groups, the ten-word group, the piece filter's lengths, an empty read, reads with N,
    palindromes, half of the reads from the reverse strand; the pair-route targets are left alone by the table"""
    for mode in ("HW", "NW"):
        for b in SC.parity_batches(mode, "distance", -1):
            lens = [len(r) for r in b["reads"]]
            if b["name"].startswith("plain"):
                assert len(set(b["target"].tolist())) == 20 and np.array_equal(SC.COMP[b["target"]], b["target"])
                assert len(b["reads"]) == int(b["name"][5:]) and 0 in lens
                continue
            assert {(m + 31) // 32 for m in lens if 0 < m <= 256} == set(range(1, 9))
            assert 300 in lens and 600 in lens and 2000 in lens and 0 in lens
            assert any(ord("N") in r.tolist() for r in b["reads"])
            assert sum(1 for r in b["reads"] if len(r) and np.array_equal(SC.rc(r), r)) >= 4
            assert len(set(b["target"].tolist())) == (4 if b["name"] == "acgt" else 5)
            assert (30_000 <= len(b["target"]) <= 60_000) if mode == "HW" else len(b["target"]) == 300
