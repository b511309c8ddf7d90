"""CPU: the surface of pairs gathered from a read batch (edlibAmdBatchPairsSetSharedWindows,
PairBatch.set_shared_windows, edlib_amd.first_hit_windows): declared, exported, bound, and a NULL batch on either side
is an error with a message rather than a crash.  What it computes is tests/test_gpu_pairs_shared.py; the kernel's
arithmetic is tests/test_pairs_gather_bytes_model.py; the window it is given is tests/test_read_windows_model.py."""
import fnmatch
import os
import re

import edlib_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "edlibAmdBatchPairsSetSharedWindows"


def test_set_shared_windows_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "edlib_amd.h")) as f:
        header = f.read()
    assert re.search(r"EDLIB_API\s+int\s+%s\s*\(\s*EdlibAmdBatch\s*\*\s*\w+\s*,\s*EdlibAmdBatch\s*\*" % NAME, header)
    with open(os.path.join(ROOT, "edlib_amd", "csrc", "exports.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    exported = re.findall(r"([\w*?]+)\s*;", text.split("global:")[1].split("local:")[0])
    assert any(fnmatch.fnmatchcase(NAME, pat) for pat in exported), exported
    assert hasattr(edlib_amd.lib(), NAME)
    assert len(getattr(edlib_amd.lib(), NAME).argtypes) == 7


def test_python_surface_exists():
    assert callable(getattr(edlib_amd.PairBatch, "set_shared_windows", None))
    assert "set_shared_windows" in edlib_amd.PairBatch.__doc__
    assert NAME in edlib_amd.PairBatch.set_shared_windows.__doc__
    assert callable(getattr(edlib_amd, "first_hit_windows", None))
    doc = edlib_amd.first_hit_windows.__doc__
    assert "-1" in doc and "Left out" in doc and "empty window" in doc


def test_null_batches_are_errors_with_a_message():
    L = edlib_amd.lib()
    assert L.edlibAmdBatchPairsSetSharedWindows(None, None, None, None, None, None, 0) != 0
    msg = edlib_amd.last_error()
    # both handles are NULL and the message says so of each (one NULL handle beside a real batch needs a device:
    # tests/test_gpu_pairs_shared.py)
    assert NAME in msg and "null pair batch" in msg and "null read batch" in msg, msg
