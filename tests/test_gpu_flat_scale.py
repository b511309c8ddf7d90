"""-m gpu: the two sizes at which a flat pair batch takes code no smaller batch reaches.

More than 65,536 units: flat_block_offsets_kernel (flat_results.hip) scans the totals of the workgroups of 256 units with
ONE workgroup, 256 totals per trip, and carries its bases into the next trip; flat_write_kernel and cigar_kernel add
blockLoc / blockAln / blockBase[u >> 8].  The second trip starts at unit 65,536.

A chunked NW store: Batch::planFlat (engine_flat.hip) cuts an NW PATH batch where its column store would pass
0xE0000000 / 8 entries, flat_descs_kernel (flat_pairs_prepare.hip) makes the store bases relative to the chunk, and
runFlatNwPaths scans and walks chunk after chunk over one store.  The smallest such batch is about 56,100 pairs of 1 kb.

Every field of every unit and both CIGAR forms against the reference (test_gpu_flat_pairs.py: _check_task / _check)."""
import functools

import numpy as np
import pytest

from edlib_amd import synth
from test_gpu_flat_pairs import _check, _check_task, _collect, _compare, _flat_launches, _reference

pytestmark = pytest.mark.gpu
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_AC = np.frombuffer(b"AC", dtype=np.uint8)
_GT = np.frombuffer(b"GT", dtype=np.uint8)
_POS_CAP = 16                                     # kFlatPosCap: end locations a flat unit keeps beside its results


# ---------------------------------------------------------------- more than 65,536 units

N_UNITS = 65536 + 256 + 3                         # a second trip of the scan, a last workgroup of three, n % 4 == 3
_SILENT = (range(512, 768), range(65536, 65792))  # whole workgroups without a location or an op byte at k = 2


def _unrelated(rng):
    """nothing within 2 in any mode, and at most 16 end locations without a threshold: disjoint alphabets, m >= 3, T <= 15"""
    m = int(rng.choice([5, 31, 33, 63, 64, 65, 70])); T = int(rng.choice([1, 4, 15], p=[0.8, 0.1, 0.1]))
    return _GT[rng.integers(0, 2, m)], _AC[rng.integers(0, 2, T)]


@functools.lru_cache(maxsize=None)
def _tiny_pairs():
    """queries of 1..70 bases, targets of 1..120: planted, unrelated, T < m and T = 1, the lengths around a block's 64 rows
    (the empty-prefix rule), few enough end locations for the start scans of HW (2 n).  No unit has more than 16 end locations in SHW or HW (asked of the reference: such a unit
    sends a LOCATIONS / PATH run to the general path, and this file is about the flat one): one that has is replaced by
    an identical pair."""
    rng = np.random.default_rng(65795)
    qs, ts = [], []
    for u in range(N_UNITS):
        m = int(rng.choice([1, 2, 5, 31, 32, 33, 63, 64, 65, 70], p=[0.03, 0.03, 0.06] + [0.88 / 7] * 7))
        T = int(rng.choice([1, max(1, m - 3), m, m + 37, m + 37, min(120, 2 * m + 11), 120]))
        if m <= 2:
            T = min(T, 12)
        t = _ACGT[rng.integers(0, 4, T)]
        if T > m and rng.random() < 0.85:
            a = int(rng.integers(0, T - m + 1))
            q = t[a:a + m].copy()
            hit = rng.random(m) < 0.04
            q[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
        elif rng.random() < 0.85:
            q = _ACGT[rng.integers(0, 4, m)]
        else:
            q, t = _unrelated(rng)
        qs.append(q); ts.append(t)
    for r in _SILENT:
        for u in r:
            qs[u], ts[u] = _unrelated(rng)
    for u in (N_UNITS - 1, 65535, 768, 511):                       # answers right beside the silent workgroups
        qs[u] = _ACGT[rng.integers(0, 4, 33)]; ts[u] = qs[u].copy()
    for mode in ("HW", "SHW"):
        many = np.nonzero(_reference(qs, ts, mode, "distance")["numLocations"] > _POS_CAP)[0]
        assert len(many) < N_UNITS // 20
        for u in many:
            ts[u] = qs[u].copy()
    return tuple(qs), tuple(ts)


@functools.lru_cache(maxsize=None)
def _tiny_pairs_answer_at_65536():
    """the second variant: the first unit of the scan's second trip has an answer, the rest of its workgroup has none"""
    qs, ts = (list(x) for x in _tiny_pairs())
    qs[65536] = np.frombuffer(b"ACGTTGCAAC", dtype=np.uint8); ts[65536] = qs[65536].copy()
    return tuple(qs), tuple(ts)


@pytest.mark.parametrize("task", ["locations", "path"])
@pytest.mark.parametrize("mode", ["NW", "SHW", "HW"])
def test_more_than_65536_units(engine, mode, task):
    qs, ts = (list(x) for x in _tiny_pairs())
    assert len(qs) == N_UNITS > 65536 and N_UNITS % 256 == 3 and N_UNITS % 4 != 0
    for k, variant in ((-1, 0), (2, 0), (2, 1)):
        if variant:
            qs, ts = (list(x) for x in _tiny_pairs_answer_at_65536())
        ref = _reference(qs, ts, mode, task, k)
        # the placement, on the reference's answers
        nloc = ref["numLocations"]; alen = np.diff(ref["alnOff"])
        assert nloc.max() <= _POS_CAP and nloc[-1] > 0 and nloc[65535] > 0
        assert mode != "HW" or nloc.sum() <= 2 * N_UNITS               # (prepareFlat: room for 2 n + 1,024 start scans)
        if k == 2:
            assert nloc[512:768].sum() == 0 and alen[512:768].sum() == 0
            assert nloc[65537:65792].sum() == 0 and alen[65537:65792].sum() == 0
            assert (nloc[65536] > 0) == bool(variant)
            assert ref["locOff"][65536] > 0 and (nloc[:65536] > 0).sum() > 256    # the bases the second trip starts from
        if task == "path":
            assert alen[-1] > 0 and ref["alnOff"][65536] > 0
        st = _check_task(engine, qs, ts, mode, task, k=k, what="65,795 units, variant %d" % variant, ref=ref)
        assert st["scan_launches"] == _flat_launches(mode, task) and st["overflow_units"] == 0, (k, variant, st)


def test_overflow_lists_beyond_unit_65536(engine):
    """HW distances: units with 59 end locations (ACAC in (AC)x60) take the overflow pool; their lists land behind the
    bases of the scan's second trip"""
    qs, ts = (list(x) for x in _tiny_pairs())
    at = (100, 65536, 65600, 65791, N_UNITS - 2)
    for u in at:
        qs[u] = np.frombuffer(b"ACAC", dtype=np.uint8); ts[u] = np.tile(np.frombuffer(b"AC", dtype=np.uint8), 60)
    st = _check(engine, qs, ts, "HW")
    assert st["overflow_units"] == len(at)
    st = _check(engine, qs, ts, "HW", k=1)
    assert st["overflow_units"] == len(at)


# ---------------------------------------------------------------- a chunked NW store

_CHUNK_CAP = 0xE0000000 // 8                      # planFlat: 8-byte entries a ring32 launch can address


def _store_entries(m, T):
    """ring32_store_entries(8, m, T) (pair_kernels.hpp): u64 entries of one unit's column store on 8-lane rings"""
    return (((T + ((m + 31) >> 5) + 1) >> 3) + 2) * 64


def _cuts(qs, ts):
    """Batch::planFlat's cut list: a chunk ends before the unit that would take it past the cap"""
    cuts, chunk = [0], 0
    for u, (q, t) in enumerate(zip(qs, ts)):
        e = _store_entries(len(q), len(t))
        if chunk + e > _CHUNK_CAP and chunk > 0:
            cuts.append(u); chunk = 0
        chunk += e
    return cuts + [len(qs)]


@functools.lru_cache(maxsize=None)
def _chunked_set():
    """about 60,000 NW pairs of 1 kb (6,000 distinct ones under a fixed permutation: generating is the slow part), cut by
    planFlat into two chunks at a unit that is a multiple of neither 4 (flat_write_kernel's and cigar_kernel's units per
    workgroup) nor 256; their reference, once"""
    bq, bt = synth.mutated_pairs(6000, 1000, seed=160, sub=0.03, ins=0.01, dele=0.01)
    order = np.concatenate([np.random.default_rng(60000 + i).permutation(6000) for i in range(10)])
    qs = [bq[i] for i in order]; ts = [bt[i] for i in order]
    while True:
        cuts = _cuts(qs, ts)
        assert len(cuts) == 3 and 50000 < cuts[1] < 60000, cuts
        if cuts[1] % 4 and cuts[1] % 256:
            break
        qs.insert(0, bq[len(qs) % 6000]); ts.insert(0, bt[len(ts) % 6000])
    return tuple(qs), tuple(ts), tuple(cuts), _reference(qs, ts, "NW", "path")


def test_chunked_nw_store(engine):
    """60,000 x 1 kb NW PATH: two chunks over one store of about 3.8 GB of device memory (469,762,048 entries of 8 bytes),
    run twice; scan_launches counts one storing scan per chunk and nothing else, so the chunk loop ran and the general path
    did not"""
    qs, ts, cuts, ref = _chunked_set()
    assert len(cuts) == 3 and cuts[1] % 4 and cuts[1] % 256
    assert ref["editDistance"].min() >= 0 and ref["editDistance"].max() <= 128     # (inside the first band level: no unit fails it)
    st = _check_task(engine, list(qs), list(ts), "NW", "path", what="two chunks, cut at %d" % cuts[1], ref=ref)
    assert st["scan_launches"] == _flat_launches("NW", "path", chunks=len(cuts) - 1)


def test_chunked_set_streamed_between_small_ones(engine):
    """set_pairs: the chunked set into an empty batch, a one-chunk set into the buffers it left, the chunked set again"""
    qs, ts, cuts, ref = _chunked_set()
    small_q, small_t = list(qs[:1100]), list(ts[:1100])
    small_ref = _reference(small_q, small_t, "NW", "path")
    b = engine.PairBatch([], [], mode="NW", task="path")
    try:
        for q, t, r, chunks, what in ((qs, ts, ref, len(cuts) - 1, "chunked"), (small_q, small_t, small_ref, 1, "1,100 pairs"),
                                      (qs, ts, ref, len(cuts) - 1, "chunked again")):
            b.set_pairs(list(q), list(t))
            st = b.run()
            _compare(_collect(b, "path"), r, "path", ("streamed", what))
            assert st["scan_launches"] == chunks, what
    finally:
        b.close()


def _splice(ref, u, one):
    """`ref` with unit u's answer replaced by the only unit of `one`"""
    out = dict(ref)
    for f in ("status", "editDistance", "numLocations", "alphabetLength", "alignmentLength", "hasEnds", "hasStarts", "hasAlignment"):
        out[f] = ref[f].copy(); out[f][u] = one[f][0]
    for off, fields in (("locOff", ("ends", "starts")), ("alnOff", ("alignment",)), ("cigExtOff", ("cigExt",)), ("cigStdOff", ("cigStd",))):
        lo, hi = int(ref[off][u]), int(ref[off][u + 1])
        for f in fields:
            new = one[f][:int(one[off][1])]
            out[f] = ref[f][:lo] + new + ref[f][hi:] if isinstance(new, bytes) else np.concatenate([ref[f][:lo], new, ref[f][hi:]])
        out[off] = ref[off].copy(); out[off][u + 1:] += int(one[off][1]) - (hi - lo)
    return out


def test_chunked_run_falls_back_after_the_first_chunk(engine):
    """an unrelated query in the second chunk fails the band level when chunk 1 has been scanned and walked: the general
    path takes the whole run, same answers"""
    qs, ts, cuts, ref = _chunked_set()
    qs, ts = list(qs), list(ts)
    u = cuts[1] + 1001
    qs[u] = synth.random_dna(5, 1000)
    one = _reference(qs, ts, "NW", "path", select=np.array([u], dtype=np.int32))
    assert one["editDistance"][0] > 128
    st = _check_task(engine, qs, ts, "NW", "path", what="unit %d diverges" % u, ref=_splice(ref, u, one))
    assert st["scan_launches"] > _flat_launches("NW", "path", chunks=len(cuts) - 1)
