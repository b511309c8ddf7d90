"""Child process of tests/test_gpu_hit_groups.py: runs hit_groups_cases.batch(<name>) once and compares every field of every
read with the reference (native thread pool of the oracle).  The parent sets EDLIB_AMD_DEBUG=1 (read when the library loads,
hence a fresh process) and reads the library's own lines from this process's stderr."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edlib_amd                          # noqa: E402
import hit_groups_cases as HC             # noqa: E402
from oracle import oracle as O            # noqa: E402

_FIELDS = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")


def reference(b):
    reads = b["reads"]
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    return O.pool_align(np.concatenate(reads), qoff, b["target"], np.array([0, len(b["target"])], dtype=np.int64), True,
                        b["mode"], "distance", -1)


def planted_cover_their_cases(b, ref):
    """the reference's answers say that the planted reads put hits where the cases want them"""
    ends_of = lambda i: ref["ends"][ref["locOff"][i]:ref["locOff"][i + 1]]
    n_ends = len(b["ends"])
    if b["nwd"] > 1:                                         # (one word: random 31-mers come as close as the planted windows)
        for i, e in zip(b["planted"][:n_ends], b["ends"]):
            assert e in ends_of(i), (i, e, ends_of(i))
        assert {e % 16 for e in b["ends"]} == set(range(16))
        assert {HC.BOUNDARY - 1, HC.BOUNDARY, HC.T - 1} <= set(b["ends"])
    for i, (start, n) in zip(b["planted"][n_ends:], (HC.HOMO, HC.DINUC)):
        e = ends_of(i)
        assert np.sum((e >= start) & (e < start + n)) > 16, (i, ref["numLocations"][i], e[:20])   # more than a slot's 16 positions
    homo = ends_of(b["planted"][n_ends])
    assert np.any(np.diff(homo) == 1)                        # equal scores in neighbouring columns


def main(name):
    b = HC.batch(name)
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    bt = edlib_amd.SharedBatch(b["reads"], b["target"], mode=b["mode"], task="distance", k=-1)
    try:
        st = bt.run()
        got = bt.results_flat()
    finally:
        bt.close()
    assert st["path"] & 1
    ref = reference(b)
    for f in _FIELDS:
        assert np.array_equal(got[f], ref[f]), f
    if "planted" in b:
        planted_cover_their_cases(b, ref)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
