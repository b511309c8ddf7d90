"""Child process of tests/test_gpu_strands.py: runs the batch strand_cases.batch(<name>) once as a both-strand batch through
the C ABI and saves results_flat(), strands() and the stats to <out> (.npz).  The parent sets EDLIB_AMD_DEBUG=1 (read when
the library loads, hence a fresh process) and reads the library's own lines from this process's stderr."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edlib_amd        # noqa: E402
import strand_cases     # noqa: E402


def main(name, out):
    b = strand_cases.batch(name)
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    B = edlib_amd.BothStrandsBatch(b["reads"], b["target"], mode=b["mode"], task=b["task"], k=b["k"])
    try:
        st = B.run()
        got = B.results_flat()
        strand, both = B.strands()
    finally:
        B.close()
    np.savez(out, stats=np.array(json.dumps(st)), strand=strand, bothStrands=both,
             **{f: v for f, v in got.items() if v is not None})
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
