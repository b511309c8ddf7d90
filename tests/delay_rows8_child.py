"""Child process of tests/test_gpu_delay_rows8.py: runs one batch of tests/delay_rows8_cases.py TWICE on one resident batch
(the last level's segment records are reused from run to run) and compares every field of every read with the reference
after each run.  The parent sets EDLIB_AMD_DEBUG=1 (read when the library loads, hence a fresh process) and reads the
library's own lines from this process's stderr."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                        # noqa: E402

import edlib_amd                          # noqa: E402
import delay_rows8_cases as DC            # noqa: E402
from oracle import oracle as O            # noqa: E402

FIELDS = ("status", "editDistance", "numLocations", "alphabetLength", "locOff", "ends", "alnOff", "alignment")


def main(name):
    b = DC.batch(name)
    reads, target = b["reads"], b["target"]
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    qoff = np.zeros(len(reads) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum([len(r) for r in reads])
    ref = O.pool_align(np.concatenate(reads), qoff, target, np.array([0, len(target)], dtype=np.int64), True, "HW", "distance", -1)
    sb = edlib_amd.SharedBatch(reads, target, mode="HW", task="distance", k=-1)
    try:
        for run in (1, 2):
            st = sb.run()
            got = sb.results_flat()
            assert st["path"] & 1
            for f in FIELDS:
                assert np.array_equal(got[f], ref[f]), (run, f)
            sys.stderr.write("[child] run %d compared\n" % run)
    finally:
        sb.close()
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
