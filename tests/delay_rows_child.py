"""Child process of tests/test_gpu_delay_rows.py: runs one batch of tests/delay_rows_cases.py (a word count, or "mixed") once
and compares every field of every read with the reference (_check of test_gpu_long_reads).  The parent sets EDLIB_AMD_DEBUG=1
(read when the library loads, hence a fresh process) and reads the library's own lines from this process's stderr."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edlib_amd                          # noqa: E402
import delay_rows_cases as DR             # noqa: E402
from test_gpu_long_reads import _check    # noqa: E402


def main(name):
    b = DR.mixed() if name == "mixed" else DR.batch(int(name))
    assert edlib_amd.device_count() >= 1, "no HIP device visible: " + edlib_amd.last_error()
    st = _check(edlib_amd, b["reads"], b["target"], "distance")
    assert st["path"] & 1
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
