"""CPU: the surface of streamed pairs (edlibAmdBatchPairsSetPairs, PairBatch.set_pairs): declared, exported, bound, and a
NULL batch is an error with a message rather than a crash.  What it computes is tests/test_gpu_pairs_stream.py."""
import fnmatch
import os
import re

import edlib_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "edlibAmdBatchPairsSetPairs"


def test_set_pairs_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "edlib_amd.h")) as f:
        header = f.read()
    assert re.search(r"EDLIB_API\s+int\s+%s\s*\(\s*EdlibAmdBatch\s*\*" % NAME, header)
    with open(os.path.join(ROOT, "edlib_amd", "csrc", "exports.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    exported = re.findall(r"([\w*?]+)\s*;", text.split("global:")[1].split("local:")[0])
    assert any(fnmatch.fnmatchcase(NAME, pat) for pat in exported), exported
    assert hasattr(edlib_amd.lib(), NAME)


def test_python_method_exists():
    assert callable(getattr(edlib_amd.PairBatch, "set_pairs", None))
    assert "set_pairs" in edlib_amd.PairBatch.__doc__


def test_null_batch_is_an_error_with_a_message():
    L = edlib_amd.lib()
    assert L.edlibAmdBatchPairsSetPairs(None, None, None, None, None, 0) != 0
    msg = edlib_amd.last_error()
    assert NAME in msg and "null" in msg.lower(), msg
