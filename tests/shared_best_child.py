"""Child process of tests/test_gpu_shared_best.py: runs one batch of tests/shared_best_cases.py (word count, row form) TWICE
on one SharedBatch, requires the two outputs to be identical array by array, and compares every field of every read with the
reference, computed once.  The parent sets EDLIB_AMD_DEBUG=1 (read when the library loads, hence a fresh process) and reads the
library's own lines from this process's stderr."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edlib_amd                          # noqa: E402
import shared_best_cases as SC            # noqa: E402
from oracle import oracle as O            # noqa: E402

FIELDS = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")


def main(nwd, form):
    b = SC.batch(nwd, form)
    reads, target = b["reads"], b["target"]
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    runs = []
    batch = edlib_amd.SharedBatch(reads, target, mode="HW", task="distance", k=-1)
    try:
        for _ in range(2):
            st = batch.run()
            assert st["path"] & 1
            got = batch.results_flat()
            runs.append({f: np.array(got[f], copy=True) for f in FIELDS})
    finally:
        batch.close()
    for f in FIELDS:
        assert np.array_equal(runs[0][f], runs[1][f]), "two runs differ in " + f
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    ref = O.pool_align(np.concatenate(reads), qoff, target, np.array([0, len(target)], dtype=np.int64), True, "HW", "distance", -1)
    for f in FIELDS:
        if not np.array_equal(runs[0][f], ref[f]):
            bad = [name for name, at in b["where"].items()
                   if f in ("editDistance", "numLocations") and runs[0][f][at] != ref[f][at]]
            raise AssertionError("%s differs from the reference (planted reads among them: %s)" % (f, bad))
    print("ok")


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
