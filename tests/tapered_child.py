"""Child process of tests/test_gpu_tapered_segments.py: runs tapered_cases.batch() twice on one resident batch and saves
results_flat() of both runs and the stats to <out> (.npz).  The parent sets EDLIB_AMD_DEBUG=1 (read when the library loads,
hence a fresh process) and reads the library's own lines from this process's stderr."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edlib_amd        # noqa: E402
import tapered_cases    # noqa: E402


def main(out):
    b = tapered_cases.batch()
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    B = edlib_amd.SharedBatch(b["reads"], b["target"], mode="HW", task="distance", k=-1)
    save = {}
    try:
        for run in (1, 2):
            st = B.run()
            got = B.results_flat()
            save["stats%d" % run] = np.array(json.dumps(st))
            for f, v in got.items():
                if v is not None:
                    save["%s%d" % (f, run)] = np.array(v)
    finally:
        B.close()
    np.savez(out, **save)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
