"""Child process of tests/test_gpu_wide_rows.py: runs the batch wide_rows_cases.case(<name>) once, compares every field of
every read with the reference (_check of test_gpu_long_reads) and prints the run's statistics as one JSON line.  The parent
sets EDLIB_AMD_DEBUG=1 (read when the library loads, hence a fresh process) and reads the library's own lines from this
process's stderr."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edlib_amd                          # noqa: E402
import wide_rows_cases as WR              # noqa: E402
from test_gpu_long_reads import _check    # noqa: E402


def main(name):
    b = WR.case(name)
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    st = _check(edlib_amd, b["reads"], b["target"], b["task"], k=b["k"])
    print("stats " + json.dumps({k: int(st[k]) for k in ("path", "overflow_units")}))
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
