"""-m gpu: a general (non-flat, non-cross) resident batch run three times.  The records of the run before last are recycled,
the scratch of the pair path and the lists of the later phases are kept from run to run: a list that is appended to without
being blanked shows up as a doubled list on the second run.  After run 1 and after run 3 both collections (the flat view and
the per-unit records) are compared field by field with the reference (native pool); the statistics of runs 2 and 3 agree."""
import os

import numpy as np
import pytest

import strand_cases as SC
from edlib_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_ALL = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "starts", "alnOff", "alignment")
_DISTANCE = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")
_STATS = ("word_steps", "scan_launches", "path", "overflow_units", "algo_bytes")


def _records_as_flat(recs, task):
    """the per-unit records of results(raw=True) in the layout of results_flat()"""
    n = len(recs)
    out = {f: np.array([r[f] for r in recs], dtype=np.int32).reshape(n) for f in ("status", "editDistance", "numLocations", "alphabetLength")}
    cat = lambda lists, dt: np.array([x for l in lists for x in l], dtype=dt)
    for r in recs:
        assert len(r["endLocations"] or []) == r["numLocations"]
        assert r["startLocations"] is None or len(r["startLocations"]) == r["numLocations"]
    out["locOff"] = np.concatenate([[0], np.cumsum(out["numLocations"], dtype=np.int64)]).astype(np.int64)
    out["ends"] = cat([r["endLocations"] or [] for r in recs], np.int32)
    # (a unit without start locations -- an empty read -- has -1 for each of its end locations in the flat layout)
    out["starts"] = cat([r["startLocations"] if r["startLocations"] is not None else [-1] * r["numLocations"] for r in recs],
                        np.int32) if task != "distance" else None
    out["alnOff"] = np.concatenate([[0], np.cumsum([r["alignmentLength"] for r in recs], dtype=np.int64)]).astype(np.int64)
    out["alignment"] = np.frombuffer(b"".join(r["alignment"] or b"" for r in recs), dtype=np.uint8)
    return out


def _same(got, ref, task, tag):
    z = np.zeros(0, dtype=np.int32)
    assert len(got["status"]) == len(ref["status"]), tag                 # (no unit unchecked)
    for f in (_DISTANCE if task == "distance" else _ALL):
        a = got[f] if got[f] is not None else z
        r = ref[f] if ref[f] is not None else z
        assert np.array_equal(a, r), (f, tag)


def _three_runs(b, ref, task, strands=None):
    """run; both collections; run twice more; both collections again -- all four against `ref`; returns the last statistics"""
    try:
        b.run()
        takes = [("run 1, view", b.results_flat()), ("run 1, records", _records_as_flat(b.results(raw=True), task))]
        if strands is not None:
            s, both = b.strands()
            assert np.array_equal(s, strands[0]) and np.array_equal(both, strands[1]), "strands after run 1"
        b.run(); st2 = b.stats()
        b.run(); st3 = b.stats()
        takes += [("run 3, view", b.results_flat()), ("run 3, records", _records_as_flat(b.results(raw=True), task))]
        if strands is not None:
            s, both = b.strands()
            assert np.array_equal(s, strands[0]) and np.array_equal(both, strands[1]), "strands after run 3"
    finally:
        b.close()
    for tag, got in takes:
        _same(got, ref, task, tag)
    for f in _STATS:
        assert st2[f] == st3[f], (f, st2[f], st3[f])
    return st3


def _offsets(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return off


def _pair_ref(qs, ts, mode, task, k):
    return O.pool_align(np.concatenate(qs), _offsets(qs), np.concatenate(ts), _offsets(ts), False, mode, task, k)


def _shared_ref(reads, target, mode, task, k=-1):
    pool, off = SC.pack(reads)
    return O.pool_align(pool, off, target, np.array([0, len(target)], dtype=np.int64), True, mode, task, k)


def _nw_pairs():
    """96 pairs of 150 .. 700 bases at 5 % edits: below the 1,024 units from which short pairs take the flat path"""
    rng = np.random.default_rng(71)
    qs, ts = [], []
    for i in range(96):
        t = _ACGT[rng.integers(0, 4, int(rng.integers(150, 701)))]
        q, _ = synth.mutate(t, int(rng.integers(1 << 30)), 0.03, 0.01, 0.01)
        qs.append(np.ascontiguousarray(q)); ts.append(np.ascontiguousarray(t))
    return qs, ts


def _hw_pairs():
    """the same shapes as HW: each query a mutated slice of its target, T = m + 200"""
    rng = np.random.default_rng(72)
    qs, ts = [], []
    for i in range(96):
        m = int(rng.integers(150, 701))
        t = _ACGT[rng.integers(0, 4, m + 200)]
        a = int(rng.integers(0, 201))
        q, _ = synth.mutate(t[a:a + m], int(rng.integers(1 << 30)), 0.03, 0.01, 0.01)
        qs.append(np.ascontiguousarray(q)); ts.append(np.ascontiguousarray(t))
    return qs, ts


def _planted(rng, target, n, m, sub, indel, flip_every=0):
    reads = []
    for i in range(n):
        a = int(rng.integers(0, len(target) - m + 1))
        q, _ = synth.mutate(target[a:a + m], int(rng.integers(1 << 30)), sub, indel, indel)
        q = np.ascontiguousarray(q)
        reads.append(SC.rc(q) if flip_every and i % flip_every == 1 else q)
    return reads


@pytest.mark.parametrize("mode,task,k", [
    ("NW", "path", -1),            # records blanked in the finalize loop; fused levels
    ("HW", "locations", -1),       # the semi-global finalize loop and phase 2
    ("NW", "distance", 10),        # records pre-filled behind the scan, then "above k"
])
def test_pair_units_only(engine, mode, task, k):
    qs, ts = _hw_pairs() if mode == "HW" else _nw_pairs()
    ref = _pair_ref(qs, ts, mode, task, k)
    if k >= 0:
        assert (ref["editDistance"] < 0).any() and (ref["editDistance"] >= 0).any()
    st = _three_runs(engine.PairBatch(qs, ts, mode=mode, task=task, k=k), ref, task)
    assert st["path"] & 2


@pytest.mark.parametrize("task", ["locations", "distance"])    # records built in the run / left on the device (lazy)
def test_reads_only(engine, task):
    rng = np.random.default_rng(73)
    target = _ACGT[rng.integers(0, 4, 20_000)]
    reads = _planted(rng, target, 200, 100, 0.02, 0.005)
    ref = _shared_ref(reads, target, "HW", task)
    st = _three_runs(engine.SharedBatch(reads, target, mode="HW", task=task), ref, task)
    assert st["path"] & 1


def test_every_unit_class_in_one_shared_batch(engine):
    """read groups, an empty read, long reads the piece filter resolves, long reads it hands back to a full-height group made
    inside the run, and one of 1,100 bases (above the 1,024 rows of that kernel) that the default plan hands on to the pair
    kernels: the run's pair units are then not the batch's"""
    saved = os.environ.pop("EDLIB_AMD_TALL_MIN_WAVES", None)
    try:
        rng = np.random.default_rng(74)
        target = _ACGT[rng.integers(0, 4, 40_000)]
        reads = _planted(rng, target, 64, 100, 0.02, 0.005)
        reads.append(np.zeros(0, dtype=np.uint8))
        reads += _planted(rng, target, 3, 600, 0.01, 0.005)
        reads += [np.ascontiguousarray(_ACGT[rng.integers(0, 4, m)]) for m in (600, 600, 1100)]
        ref = _shared_ref(reads, target, "HW", "path")
        st = _three_runs(engine.SharedBatch(reads, target, mode="HW", task="path"), ref, "path")
        assert st["path"] & 2 and st["path"] & 4, st["path"]
    finally:
        if saved is not None:
            os.environ["EDLIB_AMD_TALL_MIN_WAVES"] = saved


def test_both_strands(engine):
    rng = np.random.default_rng(75)
    target = _ACGT[rng.integers(0, 4, 20_000)]
    reads = _planted(rng, target, 32, 100, 0.02, 0.005, flip_every=2)
    reads.append(np.zeros(0, dtype=np.uint8))
    reads += _planted(rng, target, 2, 600, 0.01, 0.005, flip_every=2)
    b = {"reads": reads, "target": target, "mode": "HW", "task": "locations", "k": -1}
    ref, _ = SC.reference_both(b)
    assert ref["strand"][:32:2].sum() == 0 and ref["strand"][1:32:2].all() and ref["strand"][-1] == 1
    _three_runs(engine.BothStrandsBatch(reads, target, mode="HW", task="locations"), ref, "locations",
                strands=(ref["strand"], ref["bothStrands"]))
