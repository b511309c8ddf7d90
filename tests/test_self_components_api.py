"""CPU: the components surface of self batches (edlibAmdBatchSelfComponents) is declared, exported, bound and laid out as
documented, and what it refuses without looking at a device -- `what` 0 or with unknown bits, a NULL batch, a NULL out --
is refused with its message.  The Python entry points exist and refuse what the Creates refuse."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["numSequences", "numComponents", "label", "componentSize", "componentOffsets", "members"]


def test_header_declares_components_surface():
    src = open(os.path.join(ROOT, "include", "edlib_amd.h")).read()
    assert re.search(r"EDLIB_API\s+int\s+edlibAmdBatchSelfComponents\s*\(\s*EdlibAmdBatch\*\s*batch,\s*int\s+maxDistance,"
                     r"\s*int\s+what,\s*EdlibAmdSelfComponents\*\s*out\)", src)
    end = src.index("} EdlibAmdSelfComponents;")
    body = re.sub(r"/\*.*?\*/", "", src[src.rindex("typedef struct {", 0, end):end], flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    assert re.search(r"#define\s+EDLIB_AMD_COMPONENT_LABELS\s+1\b", src)
    assert re.search(r"#define\s+EDLIB_AMD_COMPONENT_MEMBERS\s+2\b", src)
    assert "SMALLEST index" in src                                   # the canonical label is part of the contract


def test_components_symbol_exported_and_bound():
    import edlib_amd
    L = edlib_amd.lib()
    assert hasattr(L, "edlibAmdBatchSelfComponents")
    assert L.edlibAmdBatchSelfComponents.argtypes[1:3] == [C.c_int, C.c_int]
    assert edlib_amd.COMPONENT_LABELS == 1 and edlib_amd.COMPONENT_MEMBERS == 2
    for f in ("cluster_within", "self_components_model"):
        assert callable(getattr(edlib_amd, f))
    assert callable(edlib_amd.SelfBatch.components)


def test_components_struct_layout():
    import edlib_amd
    S = edlib_amd.SelfComponents
    assert [f for f, _ in S._fields_] == FIELDS
    assert C.sizeof(S) == 8 + 4 * 8
    assert S.numSequences.offset == 0 and S.numComponents.offset == 4
    for i, n in enumerate(FIELDS[2:]):
        assert getattr(S, n).offset == 8 + 8 * i, n


@pytest.mark.parametrize("what", [0, 4, 5, 8 | 3, -1])
def test_components_refuse_unknown_parts(what):
    import edlib_amd
    L = edlib_amd.lib()
    out = edlib_amd.SelfComponents()
    assert L.edlibAmdBatchSelfComponents(None, -1, what, C.byref(out)) != 0
    err = edlib_amd.last_error()
    assert "unknown parts %d" % what in err and "EDLIB_AMD_COMPONENT_LABELS" in err


@pytest.mark.parametrize("what", [1, 2, 3])
def test_components_refuse_null(what):
    import edlib_amd
    L = edlib_amd.lib()
    assert L.edlibAmdBatchSelfComponents(None, -1, what, C.byref(edlib_amd.SelfComponents())) != 0
    assert "null" in edlib_amd.last_error()
    assert L.edlibAmdBatchSelfComponents(None, 0, what, None) != 0
    assert "null" in edlib_amd.last_error()


def test_cluster_within_python_refusals():
    import edlib_amd
    with pytest.raises(ValueError, match="strands"):
        edlib_amd.cluster_within([b"ACGT", b"ACGA"], 1, strands="sideways")
    with pytest.raises(RuntimeError, match="k >= 0"):
        edlib_amd.cluster_within([b"ACGT", b"ACGA"], -1)
