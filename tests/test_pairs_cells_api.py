"""CPU: the surface of pairs gathered from a cross or self batch (edlibAmdBatchPairsSetCells, PairBatch.set_cells,
edlib_amd.cell_windows): declared with its 8 parameters, exported, bound, and a NULL batch on either side is an error
with a message rather than a crash.  What it computes is tests/test_gpu_pairs_cells.py; the kernel's arithmetic is
tests/test_pairs_gather_cells_model.py; the windows it is given are tests/test_cell_windows_model.py."""
import fnmatch
import os
import re

import edlib_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "edlibAmdBatchPairsSetCells"


def test_set_cells_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "edlib_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"EDLIB_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % NAME, header)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8, params
    assert all(re.match(r"EdlibAmdBatch\s*\*", p) for p in params[:2]), params
    assert [p.split()[-1].lstrip("*") for p in params[2:]] == ["pairQuery", "pairTarget", "pairStart", "pairLength",
                                                               "pairStrand", "numPairs"]
    with open(os.path.join(ROOT, "edlib_amd", "csrc", "exports.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    exported = re.findall(r"([\w*?]+)\s*;", text.split("global:")[1].split("local:")[0])
    assert any(fnmatch.fnmatchcase(NAME, pat) for pat in exported), exported
    assert hasattr(edlib_amd.lib(), NAME)
    assert len(getattr(edlib_amd.lib(), NAME).argtypes) == 8


def test_python_surface_exists():
    assert callable(getattr(edlib_amd.PairBatch, "set_cells", None))
    assert "set_cells" in edlib_amd.PairBatch.__doc__ and NAME in edlib_amd.PairBatch.__doc__
    assert NAME in edlib_amd.PairBatch.set_cells.__doc__
    assert callable(getattr(edlib_amd, "cell_windows", None))
    doc = edlib_amd.cell_windows.__doc__
    assert NAME in doc and "occurrence" in doc and "Left out" in doc and "empty window" in doc


def test_null_batches_are_errors_with_a_message():
    L = edlib_amd.lib()
    assert L.edlibAmdBatchPairsSetCells(None, None, None, None, None, None, None, 0) != 0
    msg = edlib_amd.last_error()
    # both handles are NULL and the message says so of each (one NULL handle beside a real batch needs a device:
    # tests/test_gpu_pairs_cells.py)
    assert NAME in msg and "null pair batch" in msg and "null cross batch" in msg, msg
