"""-m gpu: both-strand read batches (edlibAmdBatchCreateSharedBothStrands).  Every batch is compared, read by
read and field by field, with the reference run over every read and its reverse complement (2n alignments) and resolved by
the table of tests/strand_cases.py.  The batches that prune prove it through the work counter and the library's own
EDLIB_AMD_DEBUG lines, read from a child process (tests/strand_child.py): a read whose one strand resolves in the seed pass
costs its wrong strand nothing more, and a level rescans exactly the reads that are open on both strands.
tests/test_strand_model.py checks on the CPU that every batch here is what its test assumes."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import seed_model as SM
import strand_cases as SC

pytestmark = pytest.mark.gpu

_FIELDS = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")


def _nslots(n):
    return (n + 63) // 64 * 64


def _results_flat_copies(engine, B):
    """edlibAmdBatchResultsFlat (the malloc'd copies), as the dictionary results_flat() gives"""
    L = engine.lib()
    n = B.n
    ints = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(4)]
    lo, ao = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    pe, ps, pa = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = L.edlibAmdBatchResultsFlat(B._h, ints[0].ctypes.data, ints[1].ctypes.data, ints[2].ctypes.data, ints[3].ctypes.data,
                                    lo.ctypes.data, C.byref(pe), C.byref(ps), ao.ctypes.data, C.byref(pa))
    assert rc == 0, engine.last_error()

    def take(p, count, ctype, dtype):
        if not p.value:
            return None
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(count, 1),))[:count].astype(dtype, copy=True)
        L.libc.free(p)
        return a
    out = {"status": ints[0][:n], "editDistance": ints[1][:n], "numLocations": ints[2][:n], "alphabetLength": ints[3][:n],
           "locOff": lo, "alnOff": ao, "ends": take(pe, int(lo[-1]), C.c_int, np.int32),
           "starts": take(ps, int(lo[-1]), C.c_int, np.int32), "alignment": take(pa, int(ao[-1]), C.c_ubyte, np.uint8)}
    return out


def _same_flat(got, want, task, what):
    for f in _FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)
    if task != "distance":
        # (no unit with start locations -- at most an empty read's location is there: the flat form has no starts array at all)
        assert np.array_equal(got["starts"], want["starts"]) or (got["starts"] is None and np.all(want["starts"] == -1)), (what, "starts")


def _check_both(engine, b):
    """one both-strand batch against the model: ResultsView, ResultsFlat and Results agree with it in every field, strand and
    bothStrands equal the model's, CIGARs of both formats (path), and a second Run gives the same.  Returns stats, model."""
    task = b["task"]
    want, ref2 = SC.reference_both(b, want_cigar=task == "path")
    n = len(b["reads"])
    B = engine.BothStrandsBatch(b["reads"], b["target"], mode=b["mode"], task=task, k=b["k"], additionalEqualities=b.get("eq"))
    try:
        assert B.n == n
        st = B.run()
        view = B.results_flat()
        strand, both = B.strands()
        copies = _results_flat_copies(engine, B)
        rec = B.results(raw=True)
        cig = {ext: B.cigar_list(extended=ext) for ext in (True, False)} if task == "path" else None
        B.run()
        again = B.results_flat()
        strand2, both2 = B.strands()
    finally:
        B.close()
    what = (b["name"], b["mode"], task, b["k"])
    _same_flat(view, want, task, what + ("view",))
    _same_flat(copies, want, task, what + ("flat",))
    _same_flat(again, want, task, what + ("second run",))
    assert np.array_equal(strand, want["strand"]) and np.array_equal(both, want["bothStrands"]), what
    assert np.array_equal(strand2, want["strand"]) and np.array_equal(both2, want["bothStrands"]), what
    lo, ao = want["locOff"], want["alnOff"]
    for u in range(n):
        r = rec[u]
        assert (r["status"], r["editDistance"], r["alphabetLength"]) == (want["status"][u], want["editDistance"][u], want["alphabetLength"][u]), (what, u)
        assert list(r["endLocations"] or []) == list(want["ends"][lo[u]:lo[u + 1]]), (what, u)
        if task != "distance" and r["startLocations"] is not None:
            assert list(r["startLocations"]) == list(want["starts"][lo[u]:lo[u + 1]]), (what, u)
        if task == "path":
            assert (r["alignment"] or b"") == bytes(want["alignment"][ao[u]:ao[u + 1]]), (what, u)
    if task == "path":
        for ext, offs, chars in ((True, ref2["cigExtOff"], ref2["cigExt"]), (False, ref2["cigStdOff"], ref2["cigStd"])):
            for u in range(n):
                w = int(want["unit"][u])
                assert cig[ext][u] == chars[int(offs[w]):int(offs[w + 1])].rstrip(b"\0").decode(), (what, u, ext)
    return st, want


# ------------------------------------------------------------------------------------------------- 1: parity, every route

@pytest.mark.parametrize("k", [-1, 0, 5, 40])
@pytest.mark.parametrize("task", ["distance", "locations", "path"])
def test_parity_hw(engine, task, k):
    """read groups of one to eight words and of ten, the piece filter (600 and 2,000 bases), an empty read, N, palindromes,
    unrelated reads, half of the reads from the reverse strand; targets over ACGT and over ACGT + N"""
    for b in SC.parity_batches("HW", task, k):
        st, want = _check_both(engine, b)
        assert st["cells"] == 2 * sum(len(r) for r in b["reads"]) * len(b["target"])
        if k == -1:                                                # (every read has an alignment: half of them on the reverse strand)
            assert want["strand"].sum() > 10 and (want["strand"] == 0).sum() > 10 and want["bothStrands"].sum() >= 1


@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("task", ["distance", "path"])
@pytest.mark.parametrize("mode", ["SHW", "NW"])
def test_parity_shw_nw(engine, mode, task, k):
    """the plain read groups, and the pair route: reads above 256 bases, a five-symbol target, and a 20-symbol target that the
    table leaves alone with 400 and with 1,200 reads (2,400 internal pair units)"""
    for b in SC.parity_batches(mode, task, k):
        _check_both(engine, b)


def test_parity_with_additional_equalities(engine):
    b = SC.parity_batches("HW", "locations", 5, seed=3)[0]
    b["eq"] = [("N", "A"), ("N", "C"), ("N", "G"), ("N", "T"), ("R", "A"), ("R", "G")]
    _check_both(engine, b)


def test_align_batch_both_strands(engine):
    b = SC.parity_batches("HW", "locations", -1, seed=5)[0]
    reads = b["reads"][:40]
    want, _ = SC.reference_both(dict(b, reads=reads))
    got = engine.align_batch(reads, b["target"], mode="HW", task="locations", strands="both", raw=True)
    plain = engine.align_batch(reads, b["target"], mode="HW", task="locations", raw=True)
    for u, r in enumerate(got):
        assert (r["strand"], r["bothStrands"], r["editDistance"]) == (want["strand"][u], want["bothStrands"][u], want["editDistance"][u])
        assert "strand" not in plain[u]
        if r["strand"] == 0:
            assert {f: r[f] for f in plain[u]} == plain[u]


# --------------------------------------------------------------------------------------- the library's lines, from a child

_SEED_LINE = re.compile(r"seed pass nwords=(\d+) k=(-?\d+): (\d+) of (\d+) slots handed back")
_LEVEL_LINE = re.compile(r"level kcap=(\d+): (\d+) slots rescanned")
_VIEW_LINE = re.compile(r"reads view made on the device: (\d+) units")
_STRANDS_LINE = re.compile(r"strands: (\d+) reads, forward (\d+), reverse (\d+), both (\d+), none (\d+), located (\d+)")


def _child(name, tmp_path):
    """the batch SC.batch(name) in a fresh process with EDLIB_AMD_DEBUG=1: every field, strand and bothStrands against the
    model; returns the batch, the model, the reference's 2n distances, the stats and the library's lines"""
    out = str(tmp_path / "child.npz")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "strand_child.py"), name, out],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, EDLIB_AMD_DEBUG="1"))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-800:] + p.stderr[-3000:]
    log = {"seed": {}, "levels": {}, "view": [], "strands": []}
    cur = None
    for line in p.stderr.splitlines():
        m = re.search(r"nwords=(\d+)", line)
        if m:
            cur = int(m.group(1))
        m = _SEED_LINE.search(line)
        if m:
            assert cur not in log["seed"]
            log["seed"][cur] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
        m = _LEVEL_LINE.search(line)
        if m:
            log["levels"].setdefault(cur, []).append(int(m.group(2)))
        m = _VIEW_LINE.search(line)
        if m:
            log["view"].append(int(m.group(1)))
        m = _STRANDS_LINE.search(line)
        if m:
            log["strands"].append(tuple(int(x) for x in m.groups()))
    b = SC.batch(name)
    got = np.load(out)
    want, ref2 = SC.reference_both(b)
    got = {f: got[f] if f in got.files else None for f in _FIELDS + ("starts", "strand", "bothStrands", "stats")}
    _same_flat(got, want, b["task"], name)
    assert np.array_equal(got["strand"], want["strand"]) and np.array_equal(got["bothStrands"], want["bothStrands"]), name
    st = json.loads(str(got["stats"]))
    print(name, log, st)
    return b, want, ref2["editDistance"], st, log


def _model_counts(want):
    none = int((want["editDistance"] < 0).sum())
    rev = int(want["strand"].sum())
    return (len(want["strand"]), len(want["strand"]) - rev - none, rev, int(want["bothStrands"].sum()), none)


@pytest.mark.parametrize("nwd", [5, 8])
def test_seed_pass_is_all_the_work_when_one_strand_resolves(nwd, tmp_path):
    """2: every read resolves at k_f on one strand: the work counter holds NWD word-steps per column of the model's merged
    windows over all 2n sequences and nothing else -- no level, although every wrong strand is open above k_f"""
    b, want, d2, st, log = _child("resolving:%d" % nwd, tmp_path)
    T, kf = len(b["target"]), b["kf"]
    both = SC.interleave(b["reads"])
    slots = _nslots(len(both))
    assert slots < 16_384 and slots * T >= 1 << 30
    pred = SM.predict_batch(both, b["target"], kf)
    assert sum(p["back"] for p in pred) == 0
    cols = nwd * sum(p["columns"] for p in pred)
    full = nwd * T * int(np.sum(np.minimum(d2[0::2], d2[1::2]) >= 0))              # one full-height pass over the wrong strands
    print("nwd=%d: word_steps %d, model %d, wrong strands at full height %.3g" % (nwd, st["word_steps"], cols, full))
    assert log["seed"][nwd] == (kf, 0, slots), log
    assert st["overflow_units"] == 0, st
    assert not log["levels"], log
    assert st["word_steps"] == cols, (st, cols)
    one = (d2[0::2] <= kf) ^ (d2[1::2] <= kf)                     # (k = -1: every distance is >= 0)
    assert one.sum() * 100 >= 99 * len(b["reads"])               # the other strand of nearly every read is open above k_f


@pytest.mark.parametrize("nwd", [5, 8])
def test_what_climbs_is_what_is_open_on_both_strands(nwd, tmp_path):
    """3: 5 % unrelated reads, 3 % above k_f: the one later level (fewer than 16,384 slots: the full one) rescans both slots
    of exactly the reads whose two reference distances are above k_f"""
    b, want, d2, st, log = _child("climbing:%d" % nwd, tmp_path)
    T = len(b["target"])
    m_min = min(len(r) for r in b["reads"])
    assert _nslots(2 * len(b["reads"])) < 16_384
    assert log["seed"][nwd][0] == SM.seed_threshold(m_min, T) == b["kf"]
    open_both = int(np.sum((d2[0::2] > b["kf"]) & (d2[1::2] > b["kf"])))
    assert open_both > 0 and log["levels"][nwd] == [2 * open_both], (open_both, log)


@pytest.mark.parametrize("kind", ["three", "five_n"])
def test_banded_groups_prune_too(kind, tmp_path):
    """4: no seed pass (first threshold 8 on the banded kernel); the level rescans the reads above 8 on both strands"""
    b, want, d2, st, log = _child("banded:%s" % kind, tmp_path)
    assert not log["seed"], log
    open_both = int(np.sum((d2[0::2] > 8) & (d2[1::2] > 8)))
    assert open_both > 0 and log["levels"][b["nwd"]] == [2 * open_both], (open_both, log)


def test_view_is_made_on_the_device_and_n_wide(tmp_path):
    """5: a DISTANCE batch of two word groups: the winners are gathered into read order on the device, n units come over"""
    b, want, d2, st, log = _child("two", tmp_path)
    assert log["view"] == [len(b["reads"])], log
    assert log["strands"] == [_model_counts(want) + (0,)], (log, _model_counts(want))


@pytest.mark.parametrize("task", ["locations", "path"])
def test_only_winners_are_located(task, tmp_path):
    """6: the start-location and path phases take the reported strand of every read that has an alignment, nothing else"""
    b, want, d2, st, log = _child("climbing:5:%s" % task, tmp_path)
    counts = _model_counts(want)
    located = int((want["editDistance"] >= 0).sum())
    assert located == len(b["reads"]) and counts[3] >= 0
    assert log["strands"] == [counts + (located,)], (log, counts, located)


def test_other_batches_are_untouched(engine):
    """7: edlibAmdBatchStrandView fails on a shared, a pair and a cross batch; edlibAmdBatchCrossView on a both-strand batch"""
    L = engine.lib()
    t = b"ACGTTGCATTGACCAGT" * 4
    reads = [b"TTGCATTG", b"CAATGCAA"]
    sv = engine.StrandView()
    for B in (engine.SharedBatch(reads, t), engine.PairBatch(reads, [t, t]), engine.CrossBatch(reads, [t, t])):
        try:
            B.run()
            assert L.edlibAmdBatchStrandView(B._h, C.byref(sv)) == 1
            assert "both-strand" in engine.last_error() or "cross batch" in engine.last_error()
        finally:
            B.close()
    B = engine.BothStrandsBatch(reads, t)
    try:
        assert L.edlibAmdBatchStrandView(B._h, C.byref(sv)) == 1          # before a Run
        B.run()
        cv = engine.CrossView()
        assert L.edlibAmdBatchCrossView(B._h, engine.CROSS_BEST, C.byref(cv)) == 1
        st, both = B.strands()
        assert list(st) == [0, 1] and list(both) == [0, 0]
        assert [r["editDistance"] for r in B.results()] == [0, 0]
    finally:
        B.close()
