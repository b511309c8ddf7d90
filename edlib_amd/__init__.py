"""edlib_amd -- Python front of the MI355X edit-distance engine (ctypes over the C ABI).

Mirrors the reference's Python binding (bindings/python/edlib.pyx): ``align()`` and
``getNiceAlignment()`` have the same arguments, defaults, result dictionary and
error behaviour (edlib.pyx:56-155, 158-238), so the reference's own binding tests
(bindings/python/test.py) read the same against this package.  Additive:
``align_batch()`` / ``align_pairs()`` / ``align_cross()`` / ``align_windows()`` / ``find_all()`` / ``find_all_cross()`` / ``pdist()`` /
``pairs_within()``, ``reverse_complement()``, ``cross_strands_model()`` and the resident ``SharedBatch`` / ``BothStrandsBatch`` /
``PairBatch`` / ``CrossBatch`` / ``WindowBatch`` / ``SelfBatch`` sessions over include/edlib_amd.h.

There is no CPU path in here: everything calls ``libedlib.so`` (built by
``__graft_entry__.build()`` / ``make``), and a missing library or a missing GPU
raises.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EDLIB_AMD_LIB: another build of the same C ABI (A/B timing of two builds on one box: tools/gpu_visit.sh ab)
LIB_PATH = os.environ.get("EDLIB_AMD_LIB") or os.path.join(_HERE, "libedlib.so")

EDLIB_MODE = {"NW": 0, "SHW": 1, "HW": 2}
EDLIB_TASK = {"distance": 0, "locations": 1, "path": 2}


class EqualityPair(C.Structure):          # edlib.h:92-95
    _fields_ = [("first", C.c_char), ("second", C.c_char)]


class AlignConfig(C.Structure):           # edlib.h:100-140
    _fields_ = [("k", C.c_int), ("mode", C.c_int), ("task", C.c_int),
                ("additionalEqualities", C.POINTER(EqualityPair)),
                ("additionalEqualitiesLength", C.c_int)]


class AlignResult(C.Structure):           # edlib.h:162-218
    _fields_ = [("status", C.c_int), ("editDistance", C.c_int),
                ("endLocations", C.POINTER(C.c_int)),
                ("startLocations", C.POINTER(C.c_int)),
                ("numLocations", C.c_int),
                ("alignment", C.POINTER(C.c_ubyte)),
                ("alignmentLength", C.c_int), ("alphabetLength", C.c_int)]


class BatchStats(C.Structure):            # edlib_amd.h EdlibAmdBatchStats
    _fields_ = [("run_ms", C.c_double), ("scan_ms", C.c_double), ("scan_launches", C.c_int),
                ("cells", C.c_longlong), ("word_steps", C.c_longlong), ("algo_bytes", C.c_longlong),
                ("path", C.c_int), ("overflow_units", C.c_int), ("wide_retries", C.c_int)]


class ResultsView(C.Structure):          # edlib_amd.h EdlibAmdResultsView
    _fields_ = [("numUnits", C.c_int), ("status", C.POINTER(C.c_int)), ("editDistance", C.POINTER(C.c_int)),
                ("numLocations", C.POINTER(C.c_int)), ("alphabetLength", C.POINTER(C.c_int)),
                ("locOffsets", C.POINTER(C.c_longlong)), ("endLocations", C.POINTER(C.c_int)),
                ("startLocations", C.POINTER(C.c_int)), ("alnOffsets", C.POINTER(C.c_longlong)),
                ("alignment", C.POINTER(C.c_ubyte))]


class CrossView(C.Structure):            # edlib_amd.h EdlibAmdCrossView
    _fields_ = [("numQueries", C.c_int), ("numTargets", C.c_int)] + [
        (f, C.POINTER(C.c_int)) for f in ("editDistance", "numLocations", "endLocation",
                                          "bestQuery", "bestQueryDistance", "secondQueryDistance",
                                          "bestTarget", "bestTargetDistance", "secondTargetDistance")]


class CrossHits(C.Structure):            # edlib_amd.h EdlibAmdCrossHits
    _fields_ = [("numQueries", C.c_int), ("numTargets", C.c_int), ("numHits", C.c_longlong),
                ("targetOffsets", C.POINTER(C.c_longlong))] + [
        (f, C.POINTER(C.c_int)) for f in ("query", "editDistance", "numLocations", "endLocation")]


class CrossOccurrences(C.Structure):     # edlib_amd.h EdlibAmdCrossOccurrences
    _fields_ = [("numQueries", C.c_int), ("numTargets", C.c_int), ("numHits", C.c_longlong),
                ("targetOffsets", C.POINTER(C.c_longlong))] + [
        (f, C.POINTER(C.c_int)) for f in ("query", "firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations")]


class CrossStrands(C.Structure):         # edlib_amd.h EdlibAmdCrossStrands
    _fields_ = [("numQueries", C.c_int), ("numTargets", C.c_int), ("numHits", C.c_longlong)] + [
        (f, C.POINTER(C.c_ubyte)) for f in ("cellStrand", "hitStrand", "bestQueryStrand", "bestTargetStrand")]


class ReadHits(C.Structure):             # edlib_amd.h EdlibAmdReadHits
    _fields_ = [("numUnits", C.c_int), ("numHits", C.c_longlong), ("unitOffsets", C.POINTER(C.c_longlong))] + [
        (f, C.POINTER(C.c_int)) for f in ("firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations")]


class StrandView(C.Structure):           # edlib_amd.h EdlibAmdStrandView
    _fields_ = [("numUnits", C.c_int), ("strand", C.POINTER(C.c_ubyte)), ("bothStrands", C.POINTER(C.c_ubyte))]


class WindowView(C.Structure):           # edlib_amd.h EdlibAmdWindowView
    _fields_ = [("numUnits", C.c_int), ("numQueries", C.c_int)] + [
        (f, C.POINTER(C.c_int)) for f in ("editDistance", "numLocations", "endLocation",
                                          "bestUnit", "bestDistance", "secondDistance")]


class SelfView(C.Structure):             # edlib_amd.h EdlibAmdSelfView
    _fields_ = [("numSequences", C.c_int), ("numPairs", C.c_longlong)] + [
        (f, C.POINTER(C.c_int)) for f in ("editDistance", "nearest", "nearestDistance", "secondDistance")]


class SelfHits(C.Structure):             # edlib_amd.h EdlibAmdSelfHits
    _fields_ = [("numSequences", C.c_int), ("numHits", C.c_longlong), ("rowOffsets", C.POINTER(C.c_longlong)),
                ("partner", C.POINTER(C.c_int)), ("editDistance", C.POINTER(C.c_int))]


class SelfStrands(C.Structure):          # edlib_amd.h EdlibAmdSelfStrands
    _fields_ = [("numSequences", C.c_int), ("numPairs", C.c_longlong), ("numHits", C.c_longlong)] + [
        (f, C.POINTER(C.c_ubyte)) for f in ("pairStrand", "hitStrand", "nearestStrand")]


class SelfComponents(C.Structure):       # edlib_amd.h EdlibAmdSelfComponents
    _fields_ = [("numSequences", C.c_int), ("numComponents", C.c_int)] + [
        (f, C.POINTER(C.c_int)) for f in ("label", "componentSize", "componentOffsets", "members")]


class Neighbors(C.Structure):            # edlib_amd.h EdlibAmdNeighbors
    _fields_ = [("numRows", C.c_int), ("K", C.c_int)] + [
        (f, C.POINTER(C.c_int)) for f in ("count", "neighbor", "distance")] + [("strand", C.POINTER(C.c_ubyte))]


SELF_DISTANCES = 1                        # EDLIB_AMD_SELF_DISTANCES
SELF_NEAREST = 2                          # EDLIB_AMD_SELF_NEAREST
CROSS_MATRIX = 1                          # EDLIB_AMD_CROSS_MATRIX
CROSS_BEST = 2                            # EDLIB_AMD_CROSS_BEST
WINDOW_UNITS = 1                          # EDLIB_AMD_WINDOW_UNITS
WINDOW_BEST = 2                           # EDLIB_AMD_WINDOW_BEST
COMPONENT_LABELS = 1                      # EDLIB_AMD_COMPONENT_LABELS
COMPONENT_MEMBERS = 2                     # EDLIB_AMD_COMPONENT_MEMBERS

_lib = None


def lib():
    """The loaded C-ABI library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s not found: build it with `make` or __graft_entry__.build() "
                          "(there is no Python/CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.edlibAlign.restype = AlignResult
        L.edlibAlign.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, AlignConfig]
        L.edlibNewAlignConfig.restype = AlignConfig
        L.edlibNewAlignConfig.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(EqualityPair), C.c_int]
        L.edlibDefaultAlignConfig.restype = AlignConfig
        L.edlibFreeAlignResult.argtypes = [AlignResult]
        L.edlibAlignmentToCigar.restype = C.c_void_p
        L.edlibAlignmentToCigar.argtypes = [C.c_char_p, C.c_int, C.c_int]
        L.edlibAmdDeviceCount.restype = C.c_int
        L.edlibAmdLastError.restype = C.c_char_p
        L.edlibAmdVersion.restype = C.c_char_p
        L.edlibAmdBatchCreateShared.restype = C.c_void_p
        L.edlibAmdBatchCreateShared.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                AlignConfig, C.c_int]
        L.edlibAmdBatchCreateSharedBothStrands.restype = C.c_void_p
        L.edlibAmdBatchCreateSharedBothStrands.argtypes = L.edlibAmdBatchCreateShared.argtypes
        L.edlibAmdBatchStrandView.argtypes = [C.c_void_p, C.POINTER(StrandView)]
        L.edlibAmdBatchCreateSharedHits.restype = C.c_void_p
        L.edlibAmdBatchCreateSharedHits.argtypes = L.edlibAmdBatchCreateShared.argtypes
        L.edlibAmdBatchSharedHits.argtypes = [C.c_void_p, C.POINTER(ReadHits)]
        L.edlibAmdReverseComplement.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.edlibAmdReverseComplement.restype = None
        L.edlibAmdBatchCreatePairs.restype = C.c_void_p
        L.edlibAmdBatchCreatePairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               AlignConfig, C.c_int]
        L.edlibAmdBatchCreateCross.restype = C.c_void_p
        L.edlibAmdBatchCreateCross.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               AlignConfig, C.c_int]
        L.edlibAmdBatchCrossView.argtypes = [C.c_void_p, C.c_int, C.POINTER(CrossView)]
        L.edlibAmdBatchCreateCrossHits.restype = C.c_void_p
        L.edlibAmdBatchCreateCrossHits.argtypes = L.edlibAmdBatchCreateCross.argtypes
        L.edlibAmdBatchCrossHits.argtypes = [C.c_void_p, C.POINTER(CrossHits)]
        # the both-strand entry points are bound where the library has them: an older build named by EDLIB_AMD_LIB
        # serves every other call, and these raise AttributeError where they are asked for
        if hasattr(L, "edlibAmdBatchCrossStrands"):
            L.edlibAmdBatchCreateCrossBothStrands.restype = C.c_void_p
            L.edlibAmdBatchCreateCrossBothStrands.argtypes = L.edlibAmdBatchCreateCross.argtypes
            L.edlibAmdBatchCreateCrossHitsBothStrands.restype = C.c_void_p
            L.edlibAmdBatchCreateCrossHitsBothStrands.argtypes = L.edlibAmdBatchCreateCross.argtypes
            L.edlibAmdBatchCrossStrands.argtypes = [C.c_void_p, C.c_int, C.POINTER(CrossStrands)]
        if hasattr(L, "edlibAmdBatchCrossOccurrences"):
            L.edlibAmdBatchCreateCrossOccurrences.restype = C.c_void_p
            L.edlibAmdBatchCreateCrossOccurrences.argtypes = L.edlibAmdBatchCreateCross.argtypes
            L.edlibAmdBatchCrossOccurrences.argtypes = [C.c_void_p, C.POINTER(CrossOccurrences)]
        if hasattr(L, "edlibAmdBatchCrossSetTargets"):
            L.edlibAmdBatchCrossSetTargets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.edlibAmdBatchCreateWindows.restype = C.c_void_p
        L.edlibAmdBatchCreateWindows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, AlignConfig, C.c_int]
        if hasattr(L, "edlibAmdBatchCreateWindowsStranded"):
            L.edlibAmdBatchCreateWindowsStranded.restype = C.c_void_p
            L.edlibAmdBatchCreateWindowsStranded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                             AlignConfig, C.c_int]
        L.edlibAmdBatchWindowView.argtypes = [C.c_void_p, C.c_int, C.POINTER(WindowView)]
        if hasattr(L, "edlibAmdBatchWindowsSetUnits"):
            L.edlibAmdBatchWindowsSetUnits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "edlibAmdBatchPairsSetPairs"):
            L.edlibAmdBatchPairsSetPairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "edlibAmdBatchPairsSetWindows"):
            L.edlibAmdBatchPairsSetWindows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int]
        if hasattr(L, "edlibAmdBatchPairsSetSharedWindows"):
            L.edlibAmdBatchPairsSetSharedWindows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_int]
        if hasattr(L, "edlibAmdBatchPairsSetCells"):
            L.edlibAmdBatchPairsSetCells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int]
        if hasattr(L, "edlibAmdBatchCreateSelf"):
            L.edlibAmdBatchCreateSelf.restype = C.c_void_p
            L.edlibAmdBatchCreateSelf.argtypes = [C.c_void_p, C.c_void_p, C.c_int, AlignConfig, C.c_int]
            L.edlibAmdBatchCreateSelfHits.restype = C.c_void_p
            L.edlibAmdBatchCreateSelfHits.argtypes = L.edlibAmdBatchCreateSelf.argtypes
            L.edlibAmdBatchSelfView.argtypes = [C.c_void_p, C.c_int, C.POINTER(SelfView)]
            L.edlibAmdBatchSelfHits.argtypes = [C.c_void_p, C.POINTER(SelfHits)]
        if hasattr(L, "edlibAmdBatchCreateSelfHitsGrouped"):
            L.edlibAmdBatchCreateSelfHitsGrouped.restype = C.c_void_p
            L.edlibAmdBatchCreateSelfHitsGrouped.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, AlignConfig, C.c_int]
        if hasattr(L, "edlibAmdBatchSelfStrands"):
            L.edlibAmdBatchCreateSelfBothStrands.restype = C.c_void_p
            L.edlibAmdBatchCreateSelfBothStrands.argtypes = L.edlibAmdBatchCreateSelf.argtypes
            L.edlibAmdBatchCreateSelfHitsBothStrands.restype = C.c_void_p
            L.edlibAmdBatchCreateSelfHitsBothStrands.argtypes = L.edlibAmdBatchCreateSelf.argtypes
            L.edlibAmdBatchSelfStrands.argtypes = [C.c_void_p, C.c_int, C.POINTER(SelfStrands)]
        if hasattr(L, "edlibAmdBatchSelfComponents"):
            L.edlibAmdBatchSelfComponents.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SelfComponents)]
        if hasattr(L, "edlibAmdBatchSelfNeighbors"):
            L.edlibAmdBatchSelfNeighbors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Neighbors)]
            L.edlibAmdBatchCrossNeighbors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Neighbors)]
        L.edlibAmdBatchRun.argtypes = [C.c_void_p]
        L.edlibAmdBatchResults.argtypes = [C.c_void_p, C.POINTER(AlignResult)]
        L.edlibAmdBatchResultsFlat.argtypes = [C.c_void_p] + [C.c_void_p] * 9
        L.edlibAmdBatchResultsView.argtypes = [C.c_void_p, C.POINTER(ResultsView)]
        L.edlibAmdBatchCigarView.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.edlibAmdFreeResults.argtypes = [C.POINTER(AlignResult), C.c_int]
        L.edlibAmdFreeResults.restype = None
        L.edlibAmdTrim.restype = None
        L.edlibAmdBatchStats.argtypes = [C.c_void_p, C.POINTER(BatchStats)]
        L.edlibAmdBatchDestroy.argtypes = [C.c_void_p]
        L.edlibAmdBatchDestroy.restype = None
        L.edlibAlignBatchSharedTarget.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int,
                                                  AlignConfig, C.POINTER(AlignResult)]
        L.edlibAlignBatchPairs.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                           C.POINTER(C.c_int), C.c_int, AlignConfig, C.POINTER(AlignResult)]
        L.libc = C.CDLL(None)
        L.libc.free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def device_count():
    return lib().edlibAmdDeviceCount()


def last_error():
    return lib().edlibAmdLastError().decode()


# --------------------------------------------------------------- helpers

class NeedsAlphabetMapping(Exception):
    pass


def _map_ascii_string(s):
    if isinstance(s, (bytes, bytearray)):
        return bytes(s)
    if isinstance(s, np.ndarray) and s.dtype == np.uint8:
        return s.tobytes()
    if isinstance(s, str):
        b = s.encode("utf-8")
        if len(b) == len(s):
            return b
    raise NeedsAlphabetMapping()


def _map_to_bytes(query, target, additional_equalities):
    """Arbitrary hashable symbols -> single bytes (edlib.pyx:22-53)."""
    try:
        return _map_ascii_string(query), _map_ascii_string(target), additional_equalities
    except NeedsAlphabetMapping:
        alphabet = set(query).union(set(target))
        if len(alphabet) > 256:
            raise ValueError("query and target combined have more than 256 unique values, "
                             "this is not supported.")
        mapping = {c: bytes([i]) for i, c in enumerate(alphabet)}
        q = b"".join(mapping[c] for c in query)
        t = b"".join(mapping[c] for c in target)
        if additional_equalities is not None:
            additional_equalities = [(mapping[a], mapping[b]) for a, b in additional_equalities
                                     if a in mapping and b in mapping]
        return q, t, additional_equalities


def _one_byte(x):
    if isinstance(x, (bytes, bytearray)):
        return bytes(x[:1])
    return x.encode("utf-8")[:1]


def _make_config(mode, task, k, additionalEqualities):
    cfg = lib().edlibDefaultAlignConfig()
    if k is not None:
        cfg.k = k
    if mode in EDLIB_MODE:
        cfg.mode = EDLIB_MODE[mode]
    elif isinstance(mode, int):
        cfg.mode = mode
    if task in EDLIB_TASK:
        cfg.task = EDLIB_TASK[task]
    elif isinstance(task, int):
        cfg.task = task
    keep = None
    if additionalEqualities:
        keep = (EqualityPair * len(additionalEqualities))()
        for i, (a, b) in enumerate(additionalEqualities):
            keep[i].first = _one_byte(a)
            keep[i].second = _one_byte(b)
        cfg.additionalEqualities = C.cast(keep, C.POINTER(EqualityPair))
        cfg.additionalEqualitiesLength = len(additionalEqualities)
    return cfg, keep


def cigar_from_alignment(ops, extended=True):
    """edlibAlignmentToCigar (edlib.h:268-271) on a bytes object of op codes."""
    L = lib()
    p = L.edlibAlignmentToCigar(bytes(ops), len(ops), 1 if extended else 0)
    if not p:
        return None
    s = C.string_at(p).decode()
    L.libc.free(p)
    return s


def _raw_result(r):
    """EdlibAlignResult -> dict with every C field (used by the parity tests)."""
    n = r.numLocations
    return {
        "status": r.status,
        "editDistance": r.editDistance,
        "endLocations": [r.endLocations[i] for i in range(n)] if r.endLocations else None,
        "startLocations": [r.startLocations[i] for i in range(n)] if r.startLocations else None,
        "numLocations": n,
        "alignment": bytes(bytearray(r.alignment[:r.alignmentLength])) if r.alignment else None,
        "alignmentLength": r.alignmentLength,
        "alphabetLength": r.alphabetLength,
    }


def _nice_result(raw):
    """The reference binding's dictionary (edlib.pyx:136-153)."""
    locations = []
    for i in range(max(raw["numLocations"], 0)):
        locations.append((raw["startLocations"][i] if raw["startLocations"] is not None else None,
                          raw["endLocations"][i] if raw["endLocations"] is not None else None))
    cigar = cigar_from_alignment(raw["alignment"]) if raw["alignment"] is not None else None
    return {"editDistance": raw["editDistance"], "alphabetLength": raw["alphabetLength"],
            "locations": locations, "cigar": cigar}


# ----------------------------------------------------------- public API

def align_raw(query, target, mode="NW", task="distance", k=-1, additionalEqualities=None):
    """edlibAlign() with every field of EdlibAlignResult returned (bytes in)."""
    L = lib()
    cfg, keep = _make_config(mode, task, k, additionalEqualities)
    r = L.edlibAlign(query, len(query), target, len(target), cfg)
    raw = _raw_result(r)
    L.edlibFreeAlignResult(r)
    return raw


def align(query, target, mode="NW", task="distance", k=-1, additionalEqualities=None):
    """Align query with target using edit distance (same contract as the reference's
    ``edlib.align``, edlib.pyx:56-155).  Returns {editDistance, alphabetLength,
    locations: [(start, end)], cigar}; raises on status == 1."""
    q, t, eqs = _map_to_bytes(query, target, additionalEqualities)
    raw = align_raw(q, t, mode, task, k, eqs)
    if raw["status"] == 1:
        raise Exception("There was an error.")
    return _nice_result(raw)


def reverse_complement(seq):
    """edlibAmdReverseComplement: the reverse complement of a nucleotide sequence (bytes in, bytes out; a uint8 array gives
    a uint8 array).  A<->T, C<->G, U->A, the IUPAC codes by their meaning, both cases; every other byte stays."""
    as_array = isinstance(seq, np.ndarray)
    src = np.ascontiguousarray(seq, dtype=np.uint8) if as_array else np.frombuffer(bytes(seq), dtype=np.uint8)
    out = np.empty(len(src) + 1, dtype=np.uint8)
    if len(src):
        lib().edlibAmdReverseComplement(src.ctypes.data, len(src), out.ctypes.data)
    return out[:len(src)].copy() if as_array else out[:len(src)].tobytes()


# how each extended-CIGAR op fills the three display rows: (takes a query symbol, takes a target symbol, marker)
_NICE_OPS = {"=": (True, True, "|"), "X": (True, True, "."), "I": (True, False, None), "D": (False, True, None)}


def getNiceAlignment(alignResult, query, target, gapSymbol="-"):
    """Three display rows for a result of ``align(..., task="path")``: the query and target with gap symbols
    inserted, and between them a row of '|' (match), '.' (mismatch) and gap symbols.

    Same call and result keys as the reference binding's helper (bindings/python/edlib.pyx:158-238:
    ``query_aligned`` / ``matched_aligned`` / ``target_aligned``); like it, raises ``Exception`` when the
    argument is not an ``align()`` dictionary with a CIGAR.  The rows are assembled column by column from
    the expanded CIGAR; the target row starts at the first reported start location (0 when there is none)."""
    if not isinstance(alignResult, dict) or type(alignResult) is not dict:
        raise Exception("getNiceAlignment() needs the dictionary returned by align().")
    for key in ("locations", "cigar"):
        if key not in alignResult:
            raise Exception("getNiceAlignment(): the align() result has no '%s' entry." % key)
    cigar = alignResult["cigar"]
    if not cigar:
        raise Exception("getNiceAlignment(): empty CIGAR -- run align() with task='path'.")
    runs = re.findall(r"(\d+)(\D)", cigar)
    if any(op not in _NICE_OPS for _, op in runs) or "".join(n + op for n, op in runs) != cigar:
        raise Exception("getNiceAlignment(): the CIGAR must be in the extended format (=, X, I, D only).")
    start = alignResult["locations"][0][0] if alignResult["locations"] else None
    qi, ti = 0, (start or 0)
    rows = ([], [], [])                       # query, markers, target
    for count, op in runs:
        count = int(count)
        from_q, from_t, mark = _NICE_OPS[op]
        gaps = gapSymbol * count
        rows[0].append(query[qi:qi + count] if from_q else gaps)
        rows[2].append(target[ti:ti + count] if from_t else gaps)
        rows[1].append(mark * count if mark else gaps)
        qi += count if from_q else 0
        ti += count if from_t else 0
    return {"query_aligned": "".join(rows[0]), "matched_aligned": "".join(rows[1]), "target_aligned": "".join(rows[2])}


# ------------------------------------------------------------ batches

def _pack(seqs):
    """list of bytes / uint8 arrays (or one 2-D uint8 array) -> (contiguous uint8, int64 offsets)."""
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2 and seqs.dtype == np.uint8:
        n, m = seqs.shape
        return np.ascontiguousarray(seqs).reshape(-1), np.arange(n + 1, dtype=np.int64) * m
    arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, dtype=np.uint8)
            for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    data = np.concatenate(arrs) if arrs and off[-1] > 0 else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(data), off


class _Batch:
    """A batch resident in HBM: create (upload) once, run() many times, results()."""

    def __init__(self, handle, n, keep):
        if not handle:
            raise RuntimeError("edlib_amd: batch creation failed: " + last_error())
        self._h = handle
        self.n = n
        self._keep = keep

    def run(self):
        if lib().edlibAmdBatchRun(self._h) != 0:
            raise RuntimeError("edlib_amd: run failed: " + last_error())
        return self.stats()

    def stats(self):
        s = BatchStats()
        lib().edlibAmdBatchStats(self._h, C.byref(s))
        return {f: getattr(s, f) for f, _ in BatchStats._fields_}

    def results(self, raw=True):
        L = lib()
        arr = (AlignResult * max(self.n, 1))()
        if L.edlibAmdBatchResults(self._h, arr) != 0:
            raise RuntimeError("edlib_amd: results failed: " + last_error())
        out = []
        for i in range(self.n):
            d = _raw_result(arr[i])
            L.edlibFreeAlignResult(arr[i])
            out.append(d if raw else _nice_result(d))
        return out

    def results_flat(self, copy=True):
        """Every field of every result as flat numpy arrays (edlibAmdBatchResultsView: no per-unit malloc):
        status / editDistance / numLocations / alphabetLength [n], locOff [n+1] into ends / starts
        (starts is None unless the task produced start locations), alnOff [n+1] into alignment (op bytes, None unless the
        task produced paths).  copy=False: views of the batch's own pinned memory, valid until its next run() / close()."""
        L = lib()
        n = self.n
        v = ResultsView()
        if L.edlibAmdBatchResultsView(self._h, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: results failed: " + last_error())

        def arr(ptr, count, dtype):
            if not ptr:
                return None
            if count == 0:
                return np.zeros(0, dtype=dtype)
            a = np.ctypeslib.as_array(ptr, shape=(count,))
            return a.copy() if copy else a
        loc = arr(v.locOffsets, n + 1, np.int64)
        aln = arr(v.alnOffsets, n + 1, np.int64)
        nloc, naln = int(loc[-1]), int(aln[-1])
        ends = arr(v.endLocations, nloc, np.int32)
        starts = arr(v.startLocations, nloc, np.int32)
        ops = arr(v.alignment, naln, np.uint8)
        if ops is None and naln == 0:
            ops = np.zeros(0, dtype=np.uint8)
        return {"status": arr(v.status, n, np.int32), "editDistance": arr(v.editDistance, n, np.int32),
                "numLocations": arr(v.numLocations, n, np.int32), "alphabetLength": arr(v.alphabetLength, n, np.int32),
                "locOff": loc, "ends": ends if ends is not None else np.zeros(0, dtype=np.int32), "starts": starts,
                "alnOff": aln, "alignment": ops}

    def cigars(self, extended=True, copy=True):
        """edlibAlignmentToCigar over every op string of the last run (edlibAmdBatchCigarView; made on the device for a
        batch of short pairs): (chars, off) -- the NUL-terminated strings one after the other as a uint8 array, and the
        int64 offset of every string (off[n] = all bytes)."""
        L = lib()
        pc, po = C.c_void_p(), C.c_void_p()
        if L.edlibAmdBatchCigarView(self._h, 1 if extended else 0, C.byref(pc), C.byref(po)) != 0:
            raise RuntimeError("edlib_amd: cigars failed: " + last_error())
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_longlong)), shape=(self.n + 1,))
        total = int(off[-1])
        if total == 0:                             # (a batch of zero units: there is no character to point at)
            chars = np.zeros(0, dtype=np.uint8)
        else:
            chars = np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_ubyte)), shape=(total,))
        return (chars.copy(), off.copy()) if copy else (chars, off)

    def cigar_list(self, extended=True):
        chars, off = self.cigars(extended, copy=False)
        raw = chars.tobytes()
        return [raw[int(off[i]):int(off[i + 1]) - 1].decode() for i in range(self.n)]

    def results_arrays(self):
        """editDistance / numLocations / first end location / per-unit end lists (kept for older callers;
        built from results_flat())."""
        f = self.results_flat()
        loc = f["locOff"]
        first = np.full(self.n, -2, dtype=np.int64)
        has = f["numLocations"] > 0
        first[has] = f["ends"][loc[:-1][has]]
        return {"editDistance": f["editDistance"], "numLocations": f["numLocations"], "firstEnd": first,
                "alphabetLength": f["alphabetLength"], "ends": np.split(f["ends"], loc[1:-1])}

    def close(self):
        if self._h:
            lib().edlibAmdBatchDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SharedBatch(_Batch):
    """Many queries against one target (the loop of apps/aligner/aligner.cpp:162-225).
    hits=True (edlibAmdBatchCreateSharedHits; HW, distance, k >= 0, reads up to 256 bases): hits() lists, per read, every
    maximal run of target columns that end an occurrence within k; results() is not available."""

    is_hits = False

    def __init__(self, queries, target, mode="HW", task="distance", k=-1, additionalEqualities=None, device=0, hits=False):
        qd, qo = _pack(queries)
        t = np.frombuffer(target, dtype=np.uint8) if isinstance(target, (bytes, bytearray)) else np.asarray(target, dtype=np.uint8)
        t = np.ascontiguousarray(t) if len(t) else np.zeros(1, dtype=np.uint8)
        tlen = len(target)
        cfg, keep = _make_config(mode, task, k, additionalEqualities)
        self.is_hits = bool(hits)
        create = lib().edlibAmdBatchCreateSharedHits if hits else lib().edlibAmdBatchCreateShared
        h = create(qd.ctypes.data, qo.ctypes.data, len(qo) - 1, t.ctypes.data, tlen, cfg, device)
        super().__init__(h, len(qo) - 1, keep)

    def hits(self, copy=True):
        """The hits of a hits=True batch, grouped by read in the caller's order (CSR), ascending firstEnd inside a read:
        unitOffsets int64 [n + 1] (read i: [unitOffsets[i], unitOffsets[i + 1])) and firstEnd / lastEnd / editDistance /
        endLocation / numLocations int32 [numHits], plus numHits.  copy=False: views of the batch's pinned memory, valid
        until its next run() / close()."""
        if not self.is_hits:
            raise RuntimeError("edlib_amd: not a hit-list batch: create it with hits=True (a plain batch has results())")
        v = ReadHits()
        if lib().edlibAmdBatchSharedHits(self._h, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: read hits failed: " + last_error())
        n = int(v.numHits)
        off = np.ctypeslib.as_array(v.unitOffsets, shape=(self.n + 1,))
        out = {"numHits": n, "unitOffsets": off.copy() if copy else off}
        for f in ("firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations"):
            a = np.ctypeslib.as_array(getattr(v, f), shape=(n,)) if n else np.zeros(0, dtype=np.int32)
            out[f] = a.copy() if copy and n else a
        return out

    def _no_results(self, *a, **kw):
        raise RuntimeError("edlib_amd: a hit-list batch has no per-read results: use hits()")

    def results(self, raw=True):
        return self._no_results() if self.is_hits else super().results(raw)

    def results_flat(self, copy=True):
        return self._no_results() if self.is_hits else super().results_flat(copy)

    def cigars(self, extended=True, copy=True):
        return self._no_results() if self.is_hits else super().cigars(extended, copy)


class BothStrandsBatch(_Batch):
    """Many reads against one target, each as itself and as its reverse complement (edlibAmdBatchCreateSharedBothStrands):
    unit i reports the better strand's result, ties to the forward strand; strands() says which."""

    def __init__(self, queries, target, mode="HW", task="distance", k=-1, additionalEqualities=None, device=0):
        qd, qo = _pack(queries)
        t = np.frombuffer(target, dtype=np.uint8) if isinstance(target, (bytes, bytearray)) else np.asarray(target, dtype=np.uint8)
        t = np.ascontiguousarray(t) if len(t) else np.zeros(1, dtype=np.uint8)
        tlen = len(target)
        cfg, keep = _make_config(mode, task, k, additionalEqualities)
        h = lib().edlibAmdBatchCreateSharedBothStrands(qd.ctypes.data, qo.ctypes.data, len(qo) - 1,
                                                       t.ctypes.data, tlen, cfg, device)
        super().__init__(h, len(qo) - 1, keep)

    def strands(self, copy=True):
        """(strand, bothStrands) of the last run: uint8 arrays [n]; strand 0 forward, 1 reverse complement; bothStrands 1
        where the other strand reaches the same distance.  copy=False: views of the batch's pinned memory, valid until
        its next run() / close()."""
        v = StrandView()
        if lib().edlibAmdBatchStrandView(self._h, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: strand view failed: " + last_error())
        if self.n == 0:
            return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)
        a = np.ctypeslib.as_array(v.strand, shape=(self.n,))
        b = np.ctypeslib.as_array(v.bothStrands, shape=(self.n,))
        return (a.copy(), b.copy()) if copy else (a, b)


class PairBatch(_Batch):
    """Independent (query, target) pairs.
    set_pairs(queries, targets) (edlibAmdBatchPairsSetPairs) passes another pair set through the resident batch: the
    config, the stream and every buffer that is large enough stay, the set is laid out on the device, and the batch is
    then as if created over (its config, these pairs) -- run(), then results_flat() / cigars() / results().  A streamed
    set lies inside the flat envelope (queries of 1 to 1,024 bases, targets of 1 to 65,536; with task="path" also SHW / HW
    queries up to 256 bases and no pair in the linear-space regime) and may have any count; outside it the call raises and
    the batch stays as it was.
    set_windows(window_batch, unit_query, unit_start, unit_length, unit_strand=None) (edlibAmdBatchPairsSetWindows) makes
    the same streamed set from (query, strand, window) tuples over a WindowBatch on the same device: the sequences are
    gathered on the device from its resident query pool and packed target, only the tuples cross the link, and the
    window batch stays as it was -- the mapper loop set_units, run, best(), set_windows, run, cigars().
    set_shared_windows(batch, pair_query, pair_start, pair_length, pair_strand=None)
    (edlibAmdBatchPairsSetSharedWindows) makes it from (read, strand, window) tuples over a SharedBatch or a
    BothStrandsBatch: the reads and the target windows are gathered from the read batch's resident pools, so a distance
    run, first_hit_windows(), set_shared_windows, run gives start locations and CIGARs of the first hit of every read
    that mapped, equal to the whole-target HW path answer.
    set_cells(batch, pair_query, pair_target, pair_start=None, pair_length=None, pair_strand=None)
    (edlibAmdBatchPairsSetCells) makes it from (query, target, window, strand) tuples over a CrossBatch (any kind) or a
    SelfBatch: the queries and the target windows are gathered from its resident query pool and 4-bit target pack -- the
    loop set_targets, run, hits(), cell_windows(), set_cells, run gives the locations and CIGARs of the cells a cross
    batch found without a read being sliced on the host or uploaded again."""

    def __init__(self, queries, targets, mode="NW", task="distance", k=-1, additionalEqualities=None, device=0):
        qd, qo = _pack(queries)
        td, to = _pack(targets)
        if len(qo) != len(to):
            raise ValueError("queries and targets differ in count")
        cfg, keep = _make_config(mode, task, k, additionalEqualities)
        h = lib().edlibAmdBatchCreatePairs(qd.ctypes.data, qo.ctypes.data, td.ctypes.data, to.ctypes.data,
                                           len(qo) - 1, cfg, device)
        super().__init__(h, len(qo) - 1, keep)

    def set_pairs(self, queries, targets):
        """Replace the pairs (the constructor's input forms: lists of bytes / arrays, or 2-D uint8 arrays).  Raises
        RuntimeError with last_error() on a refusal, which leaves the batch as it was.  run() before the next results."""
        qd, qo = _pack(queries)
        td, to = _pack(targets)
        if len(qo) != len(to):
            raise ValueError("queries and targets differ in count")
        if lib().edlibAmdBatchPairsSetPairs(self._h, qd.ctypes.data, qo.ctypes.data, td.ctypes.data, to.ctypes.data,
                                            len(qo) - 1) != 0:
            raise RuntimeError("edlib_amd: set_pairs failed: " + last_error())
        self.n = len(qo) - 1

    def set_windows(self, window_batch, unit_query, unit_start, unit_length, unit_strand=None):
        """Replace the pairs by pairs gathered on the device from a WindowBatch (edlibAmdBatchPairsSetWindows): pair i is
        query unit_query[i] of window_batch -- its reverse complement where unit_strand[i] == 1 -- against
        target[unit_start[i] : unit_start[i] + unit_length[i]] of its target.  The batch is then what set_pairs over the
        materialised pairs would have made; the bytes are copied, so window_batch may change or close afterwards, and it
        is itself left as it was.  Raises RuntimeError with last_error() on a refusal, which leaves the batch as it was.
        run() before the next results."""
        pad, st, n = WindowBatch._units(unit_query, unit_start, unit_length, unit_strand)
        if lib().edlibAmdBatchPairsSetWindows(self._h, getattr(window_batch, "_h", None), pad[0].ctypes.data,
                                              pad[1].ctypes.data, pad[2].ctypes.data,
                                              None if st is None else st.ctypes.data, n) != 0:
            raise RuntimeError("edlib_amd: set_windows failed: " + last_error())
        self.n = n

    def set_shared_windows(self, batch, pair_query, pair_start, pair_length, pair_strand=None):
        """Replace the pairs by pairs gathered on the device from a read batch -- a SharedBatch (hits=True included) or a
        BothStrandsBatch on the same device (edlibAmdBatchPairsSetSharedWindows): pair i is read pair_query[i] of batch --
        its reverse complement where pair_strand[i] == 1 -- against target[pair_start[i] : pair_start[i] + pair_length[i]]
        of its target.  The batch is then what set_pairs over the materialised pairs would have made; the bytes are
        copied, so the read batch may run or close afterwards, and it is itself left as it was, whether it has run or not.
        first_hit_windows() makes the tuples of the first hit of every read from the read batch's results_flat().  Raises
        RuntimeError with last_error() on a refusal, which leaves the batch as it was.  run() before the next results."""
        pad, st, n = WindowBatch._units(pair_query, pair_start, pair_length, pair_strand)
        if lib().edlibAmdBatchPairsSetSharedWindows(self._h, getattr(batch, "_h", None), pad[0].ctypes.data,
                                                    pad[1].ctypes.data, pad[2].ctypes.data,
                                                    None if st is None else st.ctypes.data, n) != 0:
            raise RuntimeError("edlib_amd: set_shared_windows failed: " + last_error())
        self.n = n


    def set_cells(self, batch, pair_query, pair_target, pair_start=None, pair_length=None, pair_strand=None):
        """Replace the pairs by pairs gathered on the device from a CrossBatch (dense, hits=True, occurrences=True,
        strands="both") or a SelfBatch on the same device (edlibAmdBatchPairsSetCells): pair i is query pair_query[i] of
        batch -- its reverse complement where pair_strand[i] == 1 -- against
        targets[pair_target[i]][pair_start[i] : pair_start[i] + pair_length[i]]; pair_start and pair_length both None: every
        pair takes its whole target.  Over a SelfBatch both indices name sequences of the one set, in any order.  The
        batch is then what set_pairs over the materialised pairs would have made; the bytes are copied, so the source may
        be given new targets, run or close afterwards, and it is itself left as it was, whether it has run or not.
        cell_windows() makes the tuples of best cells (rows of hits(), cells of matrix(), best hits).  A target that is
        not in the source's 4-bit pack (above 65,536 bases, or a set of more than 16 symbols) is refused by name: pass
        those pairs through set_pairs.  Raises RuntimeError with last_error() on a refusal, which leaves the batch as it
        was.  run() before the next results."""
        if (pair_start is None) != (pair_length is None):
            raise ValueError("pair_start and pair_length are given together or not at all")
        pq, pt = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (pair_query, pair_target))
        n = len(pq)
        if len(pt) != n:
            raise ValueError("pair_query and pair_target differ in length")
        opt = []
        for a, dt in ((pair_start, np.int32), (pair_length, np.int32), (pair_strand, np.uint8)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
                if len(a) != n:
                    raise ValueError("the tuple arrays differ in length")
                a = a if n else np.zeros(1, dtype=dt)
            opt.append(a)
        pq, pt = (a if n else np.zeros(1, dtype=np.int32) for a in (pq, pt))
        if lib().edlibAmdBatchPairsSetCells(self._h, getattr(batch, "_h", None), pq.ctypes.data, pt.ctypes.data,
                                            *(None if a is None else a.ctypes.data for a in opt), n) != 0:
            raise RuntimeError("edlib_amd: set_cells failed: " + last_error())
        self.n = n


def cell_windows(mode, query, target, editDistance, endLocation, query_lengths, target_lengths, strand=None):
    """The tuples PairBatch.set_cells (edlibAmdBatchPairsSetCells) takes for BEST CELLS of a cross batch (numpy only):
    query / target / editDistance / endLocation are equally long arrays, one entry a cell -- the rows of
    CrossBatch.hits() with the target of every row, cells of matrix(), or best hits --, with d the cell's distance and e
    its first end location; query_lengths and target_lengths are the lengths of every query and target of the batch,
    strand the cells' strand bytes of a both-strand batch (bit 0 is taken; None: all forward).  mode is the cross
    batch's.  Returns (kept, pair_query, pair_target, pair_start, pair_length, pair_strand): kept the indices of the
    cells that have a window (int64), the rest int32 / uint8 arrays over them (pair_strand None where none was given),
    with the window, per target,
      HW:  [max(0, e - m - d + 1), e]   (an alignment of cost d that ends at e starts at or behind e - m - d + 1)
      SHW: [0, e]
      NW:  the whole target.
    Over that window the PATH answer of the pair batch's mode -- distance, first end, first start, alignment -- is the
    whole target's, shifted by pair_start.  Left out: cells with distance -1, cells whose first end location is -1 (HW /
    SHW: the whole query against the empty prefix) and cells of an empty target: a streamed pair set has no empty window.
    It does NOT serve occurrence runs (CrossBatch.occurrences()): a neighbouring run of the same cell, of distance d',
    may end within d + d' columns before this run's end e, lie wholly inside [e - m - d + 1, e] and tie with or beat d
    there, so the window's answer would be the neighbour's.  For occurrences pass tuples of your own to set_cells."""
    modes = {"NW": 0, "SHW": 1, "HW": 2}
    if mode not in modes:
        raise ValueError("mode must be 'NW', 'SHW' or 'HW'")
    q, t, d, e = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (query, target, editDistance, endLocation))
    if not (len(q) == len(t) == len(d) == len(e)):
        raise ValueError("query, target, editDistance and endLocation differ in length")
    ql = np.asarray(query_lengths, dtype=np.int64).reshape(-1)
    tl = np.asarray(target_lengths, dtype=np.int64).reshape(-1)
    m, T = ql[q], tl[t]
    if mode == "NW":
        keep = (d >= 0) & (T > 0)
    else:
        keep = (d >= 0) & (e >= 0) & (T > 0)
    kept = np.flatnonzero(keep)
    q, t, d, e, m, T = (a[kept] for a in (q, t, d, e, m, T))
    if mode == "HW":
        start = np.maximum(0, e - m - d + 1)
        length = e + 1 - start
    elif mode == "SHW":
        start = np.zeros(len(kept), dtype=np.int64)
        length = e + 1
    else:
        start = np.zeros(len(kept), dtype=np.int64)
        length = T
    st = None
    if strand is not None:
        st = np.asarray(strand, dtype=np.uint8).reshape(-1)
        if len(st) != len(keep):
            raise ValueError("strand and the cells differ in length")
        st = np.ascontiguousarray(st[kept] & 1)
    return kept, q.astype(np.int32), t.astype(np.int32), start.astype(np.int32), length.astype(np.int32), st


def first_hit_windows(flat, read_lengths, strand=None):
    """The tuples PairBatch.set_shared_windows takes for the first hit of every read of a HW read batch (numpy only):
    flat is its results_flat(), read_lengths the length m of every read, strand the first array of strands() of a
    both-strand batch (None: all forward).  Returns (read, start, length, strand): int32 / int32 / int32 / uint8 arrays
    over the reads with editDistance d >= 0 and first end location e >= 0, in read order, with
    start = max(0, e - m - d + 1) and length = e + 1 - start; strand is None where none was given.  Over that window
    the HW path answer -- distance, first end, first start, alignment -- is the whole target's, shifted by start.
    Left out: reads with nothing within k (editDistance -1), and reads whose first end location is the -1 of the padded
    last block (the whole read matches the empty prefix at cost d = m: a streamed pair set has no empty window)."""
    ed = np.asarray(flat["editDistance"], dtype=np.int64)
    m = np.asarray(read_lengths, dtype=np.int64)
    if len(m) != len(ed):
        raise ValueError("read_lengths and the results differ in count")
    loc = np.asarray(flat["locOff"], dtype=np.int64)
    ends = np.asarray(flat["ends"], dtype=np.int64)
    has = (ed >= 0) & (loc[1:] > loc[:-1])
    e = np.full(len(ed), -1, dtype=np.int64)
    e[has] = ends[loc[:-1][has]]
    keep = has & (e >= 0)
    read = np.flatnonzero(keep)
    e, m, ed = e[read], m[read], ed[read]
    start = np.maximum(0, e - m - ed + 1)
    st = None if strand is None else np.ascontiguousarray(np.asarray(strand, dtype=np.uint8)[read])
    return read.astype(np.int32), start.astype(np.int32), (e + 1 - start).astype(np.int32), st


class CrossBatch(_Batch):
    """Every query against every target, distances only (edlibAmdBatchCreateCross): the loop
    ``for t in targets: for q in queries: edlib.align(q, t, mode)`` as one resident batch.  Results come as a
    matrix of shape (numTargets, numQueries) and as best hits per target and per query.
    hits=True (edlibAmdBatchCreateCrossHits, k >= 0): no matrix; hits() lists the cells within k per target.
    strands="both" (edlibAmdBatchCreateCrossBothStrands / ...HitsBothStrands): every cell is the better of the query and
    its reverse complement against the target (ties: forward); matrix(), hits() and best() describe these combined
    cells, and strands() says which strand each reports.
    occurrences=True (edlibAmdBatchCreateCrossOccurrences; HW, k >= 0, queries up to 256 bases): no matrix and no best
    hits; occurrences() lists, per target and query, every maximal run of target columns that end an occurrence of the
    query within k.  Exclusive with hits=True and strands="both".
    set_targets(targets) (edlibAmdBatchCrossSetTargets) passes another target set through the resident batch: the queries
    stay, the targets are prepared on the device, and the batch is then as if created over (its queries, these targets)
    -- run(), then the views.  A streamed set lies inside the cross kernel's envelope (targets up to 65,536 bases, at
    most 16 distinct symbols, no query above 256 bases); outside it the call raises and the batch stays as it was."""

    both_strands = False
    is_occurrences = False

    def __init__(self, queries, targets, mode="HW", k=-1, additionalEqualities=None, device=0, hits=False,
                 strands="forward", occurrences=False):
        if strands not in ("forward", "both"):
            raise ValueError("strands must be 'forward' or 'both'")
        if occurrences:
            if hits:
                raise ValueError("occurrences=True and hits=True exclude each other (two kinds of batch)")
            if strands == "both":
                raise ValueError("occurrences=True has no both-strand form: pass the reverse complements as queries of their own")
            if mode != "HW":
                raise ValueError("occurrences=True needs mode='HW'")
        qd, qo = _pack(queries)
        td, to = _pack(targets)
        cfg, keep = _make_config(mode, "distance", k, additionalEqualities)
        self.numQueries, self.numTargets = len(qo) - 1, len(to) - 1
        self.is_hits = bool(hits)
        self.both_strands = strands == "both"
        self.is_occurrences = bool(occurrences)
        if self.is_occurrences:
            create = lib().edlibAmdBatchCreateCrossOccurrences
        elif self.both_strands:
            create = lib().edlibAmdBatchCreateCrossHitsBothStrands if hits else lib().edlibAmdBatchCreateCrossBothStrands
        else:
            create = lib().edlibAmdBatchCreateCrossHits if hits else lib().edlibAmdBatchCreateCross
        h = create(qd.ctypes.data, qo.ctypes.data, self.numQueries, td.ctypes.data, to.ctypes.data, self.numTargets,
                   cfg, device)
        super().__init__(h, self.numQueries * self.numTargets, keep)

    def set_targets(self, targets):
        """Replace the targets (the constructor's input forms: a list of bytes / arrays, or one 2-D uint8 array); the
        queries stay resident.  Raises RuntimeError with last_error() on a refusal, which leaves the batch as it was.
        run() before the next view."""
        td, to = _pack(targets)
        nt = len(to) - 1
        if lib().edlibAmdBatchCrossSetTargets(self._h, td.ctypes.data, to.ctypes.data, nt) != 0:
            raise RuntimeError("edlib_amd: set_targets failed: " + last_error())
        self.numTargets = nt
        self.n = self.numQueries * nt

    def _view(self, what):
        v = CrossView()
        if lib().edlibAmdBatchCrossView(self._h, what, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: cross view failed: " + last_error())
        return v

    @staticmethod
    def _arr(ptr, shape, copy):
        if not ptr:
            return None
        if int(np.prod(shape)) == 0:
            return np.zeros(shape, dtype=np.int32)
        a = np.ctypeslib.as_array(ptr, shape=shape)
        return a.copy() if copy else a

    def matrix(self, copy=True):
        """{editDistance, numLocations, endLocation}: int32 arrays of shape (numTargets, numQueries).
        copy=False: views of the batch's pinned memory, valid until its next run() / close()."""
        if self.is_hits:
            raise RuntimeError("edlib_amd: a hit-list cross batch keeps no matrix: use hits(), or create the batch "
                               "without hits=True")
        v = self._view(CROSS_MATRIX)
        shape = (self.numTargets, self.numQueries)
        return {f: self._arr(getattr(v, f), shape, copy) for f in ("editDistance", "numLocations", "endLocation")}

    def best(self, copy=True):
        """Best hits: bestQuery / bestQueryDistance / secondQueryDistance [numTargets] and bestTarget /
        bestTargetDistance / secondTargetDistance [numQueries]; ties go to the lowest index, -1 where no cell is within k."""
        v = self._view(CROSS_BEST)
        out = {}
        for f in ("bestQuery", "bestQueryDistance", "secondQueryDistance"):
            out[f] = self._arr(getattr(v, f), (self.numTargets,), copy)
        for f in ("bestTarget", "bestTargetDistance", "secondTargetDistance"):
            out[f] = self._arr(getattr(v, f), (self.numQueries,), copy)
        return out

    def hits(self, copy=True):
        """The cells within k of a hits=True batch, grouped by target (CSR), ascending query inside a target:
        targetOffsets int64 [numTargets + 1] (target t: [targetOffsets[t], targetOffsets[t + 1])) and query /
        editDistance / numLocations / endLocation int32 [numHits].  copy=False: views of the batch's pinned memory,
        valid until its next run() / close()."""
        v = CrossHits()
        if lib().edlibAmdBatchCrossHits(self._h, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: cross hits failed: " + last_error())
        n = int(v.numHits)
        out = {"targetOffsets": self._arr(v.targetOffsets, (self.numTargets + 1,), copy).astype(np.int64, copy=False)}
        for f in ("query", "editDistance", "numLocations", "endLocation"):
            out[f] = self._arr(getattr(v, f), (n,), copy) if n else np.zeros(0, dtype=np.int32)
        return out

    def occurrences(self, copy=True):
        """The occurrences of an occurrences=True batch, grouped by target (CSR), inside a target by ascending query,
        inside a (target, query) cell by ascending firstEnd: targetOffsets int64 [numTargets + 1] and query / firstEnd /
        lastEnd / editDistance / endLocation / numLocations int32 [numHits].  copy=False: views of the batch's pinned
        memory, valid until its next run() / close()."""
        if not self.is_occurrences:
            raise RuntimeError("edlib_amd: not an occurrence batch: create it with occurrences=True")
        v = CrossOccurrences()
        if lib().edlibAmdBatchCrossOccurrences(self._h, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: cross occurrences failed: " + last_error())
        n = int(v.numHits)
        out = {"targetOffsets": self._arr(v.targetOffsets, (self.numTargets + 1,), copy).astype(np.int64, copy=False)}
        for f in ("query", "firstEnd", "lastEnd", "editDistance", "endLocation", "numLocations"):
            out[f] = self._arr(getattr(v, f), (n,), copy) if n else np.zeros(0, dtype=np.int32)
        return out

    def strands(self, copy=True, cells=True):
        """The strand bytes of a strands="both" batch (edlibAmdBatchCrossStrands), uint8: cellStrand of shape
        (numTargets, numQueries) -- or hitStrand [numHits], in the order of hits(), for a hits=True batch -- and
        bestQueryStrand [numTargets] / bestTargetStrand [numQueries] for the best() hits.  Bit 0: the cell reports the
        reverse complement; bit 1: the other strand reaches the same distance; 0 where the cell or the best is -1.
        cells=False: only the two best arrays cross the link."""
        if not self.both_strands:
            raise RuntimeError("edlib_amd: not a both-strand cross batch: create it with strands='both'")
        v = CrossStrands()
        if lib().edlibAmdBatchCrossStrands(self._h, (CROSS_MATRIX if cells else 0) | CROSS_BEST, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: cross strands failed: " + last_error())

        def arr(ptr, shape):
            if not ptr or int(np.prod(shape)) == 0:
                return np.zeros(shape, dtype=np.uint8)
            a = np.ctypeslib.as_array(ptr, shape=shape)
            return a.copy() if copy else a
        out = {}
        if cells and self.is_hits:
            out["hitStrand"] = arr(v.hitStrand, (int(v.numHits),))
        elif cells:
            out["cellStrand"] = arr(v.cellStrand, (self.numTargets, self.numQueries))
        out["bestQueryStrand"] = arr(v.bestQueryStrand, (self.numTargets,))
        out["bestTargetStrand"] = arr(v.bestTargetStrand, (self.numQueries,))
        return out

    def neighbors(self, K, max_distance=-1, copy=True):
        """The K (1..64) nearest queries of every target within max_distance (< 0: every reported cell) of the last run(),
        selected on the device (edlibAmdBatchCrossNeighbors): count int32 [numTargets], neighbor / distance int32
        [numTargets, K] in ascending order of (distance, query), -1 past count; strands="both": also strand uint8
        [numTargets, K], the cell's strand byte.  Any number of times per run().  copy=False: views of the batch's pinned
        memory, valid until its next neighbors() / run() / set_targets() / close()."""
        return _neighbors(lib().edlibAmdBatchCrossNeighbors, "cross", self, K, max_distance, copy)

    def results(self, raw=True):
        raise RuntimeError("edlib_amd: a cross batch has no per-unit results: use matrix() / best()")


def _neighbors(call, kind, batch, K, max_distance, copy):
    """A neighbours call of a self or cross batch as a dict of numpy arrays (strand: both-strand batches only)."""
    v = Neighbors()
    if call(batch._h, int(K), int(max_distance), C.byref(v)) != 0:
        raise RuntimeError("edlib_amd: %s neighbors failed: %s" % (kind, last_error()))
    rows, K = int(v.numRows), int(v.K)
    out = {"count": CrossBatch._arr(v.count, (rows,), copy)}
    for f in ("neighbor", "distance"):
        out[f] = CrossBatch._arr(getattr(v, f), (rows, K), copy)
    if batch.both_strands:
        if rows == 0 or not v.strand:
            out["strand"] = np.zeros((rows, K), dtype=np.uint8)
        else:
            a = np.ctypeslib.as_array(v.strand, shape=(rows, K))
            out["strand"] = a.copy() if copy else a
    return out


def align_cross(queries, targets, mode="HW", k=-1, additionalEqualities=None, hits=False, strands="forward"):
    """Every query against every target in one device batch: the matrix() arrays (shape (numTargets, numQueries))
    and the best() arrays of CrossBatch in one dictionary; hits=True (k >= 0): the hits() arrays instead of the matrix;
    strands="both": the cells combine both strands of every query and the strands() arrays are merged in."""
    b = CrossBatch(queries, targets, mode, k, additionalEqualities, hits=hits, strands=strands)
    try:
        b.run()
        out = b.hits() if hits else b.matrix()
        out.update(b.best())
        if b.both_strands:
            out.update(b.strands())
        return out
    finally:
        b.close()


class WindowBatch(_Batch):
    """Units over one resident target, distances only (edlibAmdBatchCreateWindows): unit u is query unit_query[u]
    against target[unit_start[u] : unit_start[u] + unit_length[u]] -- the loop
    ``for read, (s, e) in candidates: edlib.align(read, ref[s:e], mode)`` as one resident batch that holds the target
    and every query once.  units() has the three fields of every unit, best() the best unit per query.
    unit_strand (edlibAmdBatchCreateWindowsStranded): 0 / 1 per unit, 1 = the unit is the reverse complement of its query
    against the window; best() runs over all units of a query whatever their strand.
    set_units(queries, unit_query, unit_start, unit_length, unit_strand=None) (edlibAmdBatchWindowsSetUnits) passes the
    next chunk of reads and candidates through the resident batch: the target, its pack and the batch's buffers stay, the
    queries and units are prepared on the device, and the batch is then as if created over (its target, these queries,
    these units) -- run(), then the views.  A streamed set lies inside the window kernel's envelope (a target of at most
    16 distinct symbols, queries up to 256 bases, windows up to 65,536 columns); outside it the call raises and the
    batch stays as it was."""

    @staticmethod
    def _units(unit_query, unit_start, unit_length, unit_strand):
        """the unit arrays as the C calls take them (an empty one padded to one element) and their count; the strand
        array is None where unit_strand is"""
        uq, us, ul = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (unit_query, unit_start, unit_length))
        if not (len(uq) == len(us) == len(ul)):
            raise ValueError("unit_query, unit_start and unit_length differ in length")
        pad = [a if len(a) else np.zeros(1, dtype=np.int32) for a in (uq, us, ul)]
        st = None
        if unit_strand is not None:
            st = np.ascontiguousarray(unit_strand, dtype=np.uint8).reshape(-1)
            if len(st) != len(uq):
                raise ValueError("unit_strand and unit_query differ in length")
            st = st if len(st) else np.zeros(1, dtype=np.uint8)
        return pad, st, len(uq)

    def __init__(self, queries, target, unit_query, unit_start, unit_length, mode="HW", k=-1,
                 additionalEqualities=None, device=0, unit_strand=None):
        qd, qo = _pack(queries)
        t = np.frombuffer(target, dtype=np.uint8) if isinstance(target, (bytes, bytearray)) else np.asarray(target, dtype=np.uint8)
        tlen = len(t)
        t = np.ascontiguousarray(t) if tlen else np.zeros(1, dtype=np.uint8)
        pad, st, nu = self._units(unit_query, unit_start, unit_length, unit_strand)
        cfg, keep = _make_config(mode, "distance", k, additionalEqualities)
        self.numQueries, self.numUnits = len(qo) - 1, nu
        if st is None:
            h = lib().edlibAmdBatchCreateWindows(qd.ctypes.data, qo.ctypes.data, self.numQueries, t.ctypes.data, tlen,
                                                 pad[0].ctypes.data, pad[1].ctypes.data, pad[2].ctypes.data,
                                                 self.numUnits, cfg, device)
        else:
            h = lib().edlibAmdBatchCreateWindowsStranded(qd.ctypes.data, qo.ctypes.data, self.numQueries, t.ctypes.data,
                                                         tlen, pad[0].ctypes.data, pad[1].ctypes.data,
                                                         pad[2].ctypes.data, st.ctypes.data, self.numUnits, cfg, device)
        super().__init__(h, self.numUnits, keep)

    def set_units(self, queries, unit_query, unit_start, unit_length, unit_strand=None):
        """Replace the queries and the units (the constructor's input forms); the target stays resident.  Raises
        RuntimeError with last_error() on a refusal, which leaves the batch as it was.  run() before the next view."""
        qd, qo = _pack(queries)
        pad, st, nu = self._units(unit_query, unit_start, unit_length, unit_strand)
        nq = len(qo) - 1
        if lib().edlibAmdBatchWindowsSetUnits(self._h, qd.ctypes.data, qo.ctypes.data, nq, pad[0].ctypes.data,
                                              pad[1].ctypes.data, pad[2].ctypes.data,
                                              None if st is None else st.ctypes.data, nu) != 0:
            raise RuntimeError("edlib_amd: set_units failed: " + last_error())
        self.numQueries, self.numUnits, self.n = nq, nu, nu

    def _view(self, what):
        v = WindowView()
        if lib().edlibAmdBatchWindowView(self._h, what, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: window view failed: " + last_error())
        return v

    def units(self, copy=True):
        """{editDistance, numLocations, endLocation}: int32 arrays [numUnits]; endLocation is the first end location of
        the unit's call, relative to its window (-1: none).  copy=False: views of the batch's pinned memory, valid
        until its next run() / close()."""
        v = self._view(WINDOW_UNITS)
        return {f: CrossBatch._arr(getattr(v, f), (self.numUnits,), copy)
                for f in ("editDistance", "numLocations", "endLocation")}

    def best(self, copy=True):
        """{bestUnit, bestDistance, secondDistance}: int32 arrays [numQueries] over the units that name each query; ties
        go to the lowest unit index, -1 where the query has no unit within k."""
        v = self._view(WINDOW_BEST)
        return {f: CrossBatch._arr(getattr(v, f), (self.numQueries,), copy)
                for f in ("bestUnit", "bestDistance", "secondDistance")}

    def results(self, raw=True):
        raise RuntimeError("edlib_amd: a window batch has no per-unit result records: use units() / best()")


def align_windows(queries, target, unit_query, unit_start, unit_length, mode="HW", k=-1, additionalEqualities=None,
                  unit_strand=None):
    """[align(queries[q], target[s:s + n], mode) for q, s, n in zip(unit_query, unit_start, unit_length)] in one device
    batch: the units() and best() arrays of WindowBatch in one dictionary.  unit_strand: 1 where the unit is
    reverse_complement(queries[q]) against its window."""
    b = WindowBatch(queries, target, unit_query, unit_start, unit_length, mode, k, additionalEqualities,
                    unit_strand=unit_strand)
    try:
        b.run()
        out = b.units()
        out.update(b.best())
        return out
    finally:
        b.close()


class SelfBatch(_Batch):
    """One set against itself, NW distances only (edlibAmdBatchCreateSelf): the loop
    ``for i: for j > i: edlib.align(seqs[i], seqs[j], "NW")`` as one resident batch that computes every unordered pair
    once.  condensed() is the int32 vector of the n (n - 1) / 2 distances in scipy's pdist order (-1: above k),
    nearest() the nearest other sequence of each.  hits=True (edlibAmdBatchCreateSelfHits, k >= 0): no vector; hits()
    lists the pairs i < j within k.
    strands="both" (edlibAmdBatchCreateSelfBothStrands / ...HitsBothStrands): pair (i, j), i < j, is the better of seqs[i]
    and reverse_complement(seqs[i]) against seqs[j] (ties: forward); condensed(), hits() and nearest() describe these
    combined distances, and strands() says which orientation each reports.
    groups= (hits=True, k >= 0; edlibAmdBatchCreateSelfHitsGrouped): an int label per sequence; only the pairs of
    sequences with equal labels exist, and hits(), nearest(), components(), neighbors() and a pair batch's set_cells()
    report what a SelfBatch(hits=True) over each group alone would, in the indices of the whole set."""

    both_strands = False
    grouped = False

    def __init__(self, seqs, k=-1, additionalEqualities=None, device=0, hits=False, strands="forward", groups=None):
        if strands not in ("forward", "both"):
            raise ValueError("strands must be 'forward' or 'both'")
        if groups is not None:
            self._init_grouped(seqs, k, additionalEqualities, device, hits, strands, groups)
            return
        sd, so = _pack(seqs)
        cfg, keep = _make_config("NW", "distance", k, additionalEqualities)
        self.numSequences = len(so) - 1
        self.numPairs = self.numSequences * (self.numSequences - 1) // 2
        self.is_hits = bool(hits)
        self.both_strands = strands == "both"
        if self.both_strands:
            create = lib().edlibAmdBatchCreateSelfHitsBothStrands if hits else lib().edlibAmdBatchCreateSelfBothStrands
        else:
            create = lib().edlibAmdBatchCreateSelfHits if hits else lib().edlibAmdBatchCreateSelf
        h = create(sd.ctypes.data, so.ctypes.data, self.numSequences, cfg, device)
        super().__init__(h, self.numPairs, keep)

    def _init_grouped(self, seqs, k, additionalEqualities, device, hits, strands, groups):
        if not hits:
            raise ValueError("groups= needs hits=True: there is no dense grouped form (a condensed vector has no meaning "
                             "across groups)")
        if k is None or k < 0:
            raise ValueError("groups= needs k >= 0: a grouped self batch is a hit list of the pairs within k")
        if strands != "forward":
            raise ValueError("groups= is one-strand: run a SelfBatch(strands='both') per group")
        sd, so = _pack(seqs)
        labels = np.asarray(groups)
        if labels.ndim != 1 or len(labels) != len(so) - 1 or (len(labels) and labels.dtype.kind not in "iu"):
            raise ValueError("groups must be a 1-D int array with one label per sequence")
        if len(labels) and (labels.min() < -2**31 or labels.max() > 2**31 - 1):
            raise ValueError("groups: labels must fit an int32 (relabel them with np.unique(groups, return_inverse=True))")
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        cfg, keep = _make_config("NW", "distance", k, additionalEqualities)
        self.numSequences = len(so) - 1
        size = np.unique(labels, return_counts=True)[1].astype(np.int64)
        self.numPairs = int((size * (size - 1) // 2).sum())            # the pairs inside groups
        self.is_hits, self.both_strands, self.grouped = True, False, True
        h = lib().edlibAmdBatchCreateSelfHitsGrouped(sd.ctypes.data, so.ctypes.data, self.numSequences,
                                                     labels.ctypes.data if len(labels) else None, cfg, device)
        _Batch.__init__(self, h, self.numPairs, keep)

    def _view(self, what):
        v = SelfView()
        if lib().edlibAmdBatchSelfView(self._h, what, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: self view failed: " + last_error())
        return v

    def condensed(self, copy=True):
        """The distances of the pairs i < j, int32 [n (n - 1) / 2], pair (i, j) at condensed_index(n, i, j).
        copy=False: a view of the batch's pinned memory, valid until its next run() / close()."""
        if self.grouped:
            raise RuntimeError("edlib_amd: condensed(): a grouped self batch keeps no condensed vector (it has no meaning "
                               "across groups): use hits()")
        if self.is_hits:
            raise RuntimeError("edlib_amd: a hit-list self batch keeps no condensed vector: use hits(), or create the "
                               "batch without hits=True")
        return CrossBatch._arr(self._view(SELF_DISTANCES).editDistance, (self.numPairs,), copy)

    def nearest(self, copy=True):
        """{nearest, nearestDistance, secondDistance}: int32 [n], over all other sequences; ties go to the lowest index,
        -1 where no other sequence is within k."""
        v = self._view(SELF_NEAREST)
        return {f: CrossBatch._arr(getattr(v, f), (self.numSequences,), copy)
                for f in ("nearest", "nearestDistance", "secondDistance")}

    def hits(self, copy=True):
        """The pairs within k of a hits=True batch, each once: rowOffsets int64 [n + 1] (partners of i:
        [rowOffsets[i], rowOffsets[i + 1])) and partner (j > i, ascending inside a row) / editDistance int32 [numHits]."""
        v = SelfHits()
        if lib().edlibAmdBatchSelfHits(self._h, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: self hits failed: " + last_error())
        n = int(v.numHits)
        out = {"rowOffsets": CrossBatch._arr(v.rowOffsets, (self.numSequences + 1,), copy).astype(np.int64, copy=False)}
        for f in ("partner", "editDistance"):
            out[f] = CrossBatch._arr(getattr(v, f), (n,), copy) if n else np.zeros(0, dtype=np.int32)
        return out

    def strands(self, copy=True, pairs=True):
        """The strand bytes of a strands="both" batch (edlibAmdBatchSelfStrands), uint8: pairStrand [n (n - 1) / 2] in
        condensed order -- or hitStrand [numHits], in the order of hits(), for a hits=True batch -- and nearestStrand [n],
        the byte of the pair (x, nearest[x]).  Bit 0: the pair reports the reverse orientation; bit 1: the other
        orientation reaches the same distance; 0 where the distance or the nearest is -1.
        pairs=False: only nearestStrand crosses the link."""
        if not self.both_strands:
            raise RuntimeError("edlib_amd: not a both-strand self batch: create it with strands='both'")
        v = SelfStrands()
        if lib().edlibAmdBatchSelfStrands(self._h, (SELF_DISTANCES if pairs else 0) | SELF_NEAREST, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: self strands failed: " + last_error())

        def arr(ptr, count):
            if not ptr or count == 0:
                return np.zeros(count, dtype=np.uint8)
            a = np.ctypeslib.as_array(ptr, shape=(count,))
            return a.copy() if copy else a
        out = {}
        if pairs and self.is_hits:
            out["hitStrand"] = arr(v.hitStrand, int(v.numHits))
        elif pairs:
            out["pairStrand"] = arr(v.pairStrand, self.numPairs)
        out["nearestStrand"] = arr(v.nearestStrand, self.numSequences)
        return out

    def components(self, max_distance=-1, members=False, copy=True):
        """The connected components of the pairs within max_distance (< 0: the batch's k) of the last run(), labelled on
        the device (edlibAmdBatchSelfComponents): label int32 [n], the smallest index in each sequence's component;
        componentSize int32 [n]; numComponents; members=True: also componentOffsets int32 [numComponents + 1] and
        members int32 [n], the components in ascending order of their labels with the members ascending inside each.
        Any number of times per run(), at any level up to k.  copy=False: views of the batch's pinned memory, valid until
        its next components() / run() / close()."""
        v = SelfComponents()
        what = COMPONENT_LABELS | (COMPONENT_MEMBERS if members else 0)
        if lib().edlibAmdBatchSelfComponents(self._h, int(max_distance), what, C.byref(v)) != 0:
            raise RuntimeError("edlib_amd: self components failed: " + last_error())
        n, nc = self.numSequences, int(v.numComponents)

        def arr(ptr, count):
            return CrossBatch._arr(ptr, (count,), copy) if count else np.zeros(0, dtype=np.int32)
        out = {"label": arr(v.label, n), "componentSize": arr(v.componentSize, n), "numComponents": nc}
        if members:
            out["componentOffsets"] = arr(v.componentOffsets, nc + 1)
            out["members"] = arr(v.members, n)
        return out

    def neighbors(self, K, max_distance=-1, copy=True):
        """The K (1..64) nearest other sequences of every sequence within max_distance (< 0: every reported pair) of the last
        run(), selected on the device (edlibAmdBatchSelfNeighbors): count int32 [n], neighbor / distance int32 [n, K] in
        ascending order of (distance, index), -1 past count; strands="both": also strand uint8 [n, K], the pair's strand
        byte.  With max_distance=-1 the columns 0 and 1 repeat nearest().  Any number of times per run().  copy=False:
        views of the batch's pinned memory, valid until its next neighbors() / run() / close()."""
        return _neighbors(lib().edlibAmdBatchSelfNeighbors, "self", self, K, max_distance, copy)

    def results(self, raw=True):
        raise RuntimeError("edlib_amd: a self batch has no per-unit results: use condensed() / hits() / nearest()")


def pdist(seqs, k=-1, additionalEqualities=None, strands="forward"):
    """NW edit distances of every pair of seqs in one device batch: the int32 condensed vector of
    scipy.spatial.distance.pdist's order (squareform() makes the matrix); -1 where a distance is above k >= 0.
    strands="both": every pair in its better orientation (SelfBatch)."""
    b = SelfBatch(seqs, k, additionalEqualities, strands=strands)
    try:
        b.run()
        return b.condensed()
    finally:
        b.close()


def pairs_within(seqs, k, additionalEqualities=None, strands="forward"):
    """Every pair i < j of seqs within k NW edits, each once, and the nearest other sequence of each, in one device batch:
    the hits() and nearest() arrays of SelfBatch(..., hits=True) in one dictionary; strands="both": in either
    orientation, with the strands() arrays merged in."""
    b = SelfBatch(seqs, k, additionalEqualities, hits=True, strands=strands)
    try:
        b.run()
        out = b.hits()
        out.update(b.nearest())
        if b.both_strands:
            out.update(b.strands())
        return out
    finally:
        b.close()


def cluster_within(seqs, k, additionalEqualities=None, strands="forward", groups=None):
    """Single linkage at k NW edits in one device batch: label int32 [n], the smallest index among the sequences that
    sequence i reaches through pairs within k (strands="both": in either orientation).  The pairs stay on the device
    (SelfBatch(..., hits=True).components()).  groups=: an int label per sequence; only pairs inside a group link."""
    b = SelfBatch(seqs, k, additionalEqualities, hits=True, strands=strands, groups=groups)
    try:
        b.run()
        return b.components()["label"]
    finally:
        b.close()


def knn(seqs, K, k=-1, additionalEqualities=None, strands="forward", groups=None):
    """The K nearest other sequences of every sequence of seqs by NW edit distance, in one device batch: the neighbors()
    arrays of SelfBatch.  k >= 0: only partners within k count, through the hit-list batch (no condensed vector is kept);
    k < 0: over all pairs, through the dense batch.  strands="both": every pair in its better orientation.
    groups=: an int label per sequence; only the other sequences of its own group count, and k must be >= 0."""
    if groups is not None and k < 0:
        raise ValueError("knn(groups=...) needs k >= 0: k < 0 would take the dense form, which a grouped batch does not have")
    b = SelfBatch(seqs, k, additionalEqualities, hits=k >= 0, strands=strands, groups=groups)
    try:
        b.run()
        return b.neighbors(K)
    finally:
        b.close()


def condensed_index(n, i, j):
    """Where pair (i, j), i != j, of n sequences sits in a condensed vector (scalars or integer arrays)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    at = np.int64(n) * lo - lo * (lo + 1) // 2 + (hi - lo - 1)
    return int(at) if at.ndim == 0 else at


def self_nearest_model(n, first, second, ed):
    """The nearest rules of a self batch stated in numpy (what SelfBatch.nearest() must equal): first / second / ed list
    pairs of different sequences, each unordered pair at most once in either orientation, with their distances (-1:
    not within k).  Per sequence, over its partners within k on either side, the smallest key (distance << 32) | partner
    is the nearest; the second distance is the smallest distance over its other partners; -1 where there is none."""
    a = np.asarray(first, dtype=np.int64).reshape(-1)
    b = np.asarray(second, dtype=np.int64).reshape(-1)
    d = np.asarray(ed, dtype=np.int64).reshape(-1)
    keep = d >= 0
    owner = np.concatenate([a[keep], b[keep]])
    partner = np.concatenate([b[keep], a[keep]])
    key = (np.concatenate([d[keep], d[keep]]) << 32) | partner
    out = {f: np.full(n, -1, dtype=np.int32) for f in ("nearest", "nearestDistance", "secondDistance")}
    order = np.lexsort((key, owner))                    # by sequence, then by key
    o, key = owner[order], key[order]
    lead = np.nonzero(np.concatenate([[True], o[1:] != o[:-1]]))[0] if len(o) else np.zeros(0, dtype=np.int64)
    out["nearest"][o[lead]] = key[lead] & 0xffffffff
    out["nearestDistance"][o[lead]] = key[lead] >> 32
    has2 = lead + 1 < len(o)
    has2[has2] = o[lead[has2] + 1] == o[lead[has2]]
    out["secondDistance"][o[lead[has2]]] = key[lead[has2] + 1] >> 32
    return out


def grouped_hits_model(groups, per_group_hits):
    """The index mapping of a grouped self batch stated in numpy (what SelfBatch(groups=...).hits() must equal): groups is
    the label array [n]; per_group_hits maps a label to the hits() dictionary of a SelfBatch(hits=True) over
    seqs[np.flatnonzero(groups == label)] alone (a missing label: no hits).  Member x of that group is sequence
    np.flatnonzero(groups == label)[x] of the whole set; members ascend, so a row's partners stay ascending."""
    g = np.asarray(groups).reshape(-1)
    n = len(g)
    rows, partner, ed = [], [], []
    for label in np.unique(g):
        h = per_group_hits.get(int(label))
        if h is None:
            continue
        member = np.flatnonzero(g == label)
        off = np.asarray(h["rowOffsets"], dtype=np.int64)
        rows.append(member[np.repeat(np.arange(len(member)), np.diff(off))])
        partner.append(member[np.asarray(h["partner"], dtype=np.int64)])
        ed.append(np.asarray(h["editDistance"], dtype=np.int32))
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    partner = np.concatenate(partner) if partner else np.zeros(0, dtype=np.int64)
    ed = np.concatenate(ed) if ed else np.zeros(0, dtype=np.int32)
    order = np.lexsort((partner, rows))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    return {"rowOffsets": off, "partner": partner[order].astype(np.int32), "editDistance": ed[order].astype(np.int32)}


def self_components_model(n, rowOffsets, partner, editDistance, level):
    """The component rules of a self batch stated in plain Python (what SelfBatch.components(level, members=True) must
    equal): rowOffsets / partner / editDistance list pairs as hits() does (CSR by the first sequence; a condensed vector
    goes in as rowOffsets = the triangle's).  A pair is an edge where its distance d is 0 <= d and, with level >= 0,
    d <= level.  Union by minimum: the root of a component is its smallest index, whatever the order of the edges."""
    off = np.asarray(rowOffsets, dtype=np.int64).reshape(-1)
    p = np.asarray(partner, dtype=np.int64).reshape(-1)
    d = np.asarray(editDistance, dtype=np.int64).reshape(-1)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(off)) if n else np.zeros(0, dtype=np.int64)
    keep = (d >= 0) & ((d <= level) if level >= 0 else True)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(row[keep].tolist(), p[keep].tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.array([find(x) for x in range(n)], dtype=np.int32)
    count = np.bincount(label, minlength=n) if n else np.zeros(0, dtype=np.int64)
    order = np.lexsort((np.arange(n), label)).astype(np.int32)           # by label, then by index
    roots = np.flatnonzero(label == np.arange(n))
    offsets = np.concatenate([[0], np.cumsum(count[roots])]).astype(np.int32)
    return {"label": label, "componentSize": count[label].astype(np.int32), "numComponents": int(len(roots)),
            "componentOffsets": offsets, "members": order}


def neighbors_model(numRows, row, partner, distance, K, level):
    """The neighbour rules of a self or cross batch stated in numpy (what neighbors(K, level) must equal): row / partner /
    distance list the candidates, entry e a candidate `partner[e]` of row `row[e]` (a self batch's pair goes in twice, once
    under each end; a partner at most once per row).  A candidate takes part where its distance d is 0 <= d and, with
    level >= 0, d <= level; a row reports its K smallest keys (distance << 32) | partner in ascending order.
    {count [numRows], neighbor [numRows, K], distance [numRows, K]}, -1 past count."""
    r = np.asarray(row, dtype=np.int64).reshape(-1)
    p = np.asarray(partner, dtype=np.int64).reshape(-1)
    d = np.asarray(distance, dtype=np.int64).reshape(-1)
    keep = (d >= 0) & ((d <= level) if level >= 0 else True)
    r, p, d = r[keep], p[keep], d[keep]
    order = np.lexsort((p, d, r))                       # by row, then by distance, then by partner
    r, p, d = r[order], p[order], d[order]
    start = np.searchsorted(r, np.arange(numRows))      # the first entry of every row
    rank = np.arange(len(r)) - start[r] if len(r) else np.zeros(0, dtype=np.int64)
    out = {"count": np.minimum(np.bincount(r, minlength=numRows), K).astype(np.int32) if numRows else np.zeros(0, dtype=np.int32),
           "neighbor": np.full((numRows, K), -1, dtype=np.int32), "distance": np.full((numRows, K), -1, dtype=np.int32)}
    top = rank < K
    out["neighbor"][r[top], rank[top]] = p[top]
    out["distance"][r[top], rank[top]] = d[top]
    return out


def window_best_model(unit_query, ed, numQueries):
    """The best-unit rules of a window batch stated in numpy (what WindowBatch.best() must equal): per query, over the
    units that name it and are within k (ed != -1), the smallest key (distance << 32) | unit index is the best; the
    second distance is the smallest distance over the query's other units; -1 where there is none."""
    uq = np.asarray(unit_query, dtype=np.int64).reshape(-1)
    ed = np.asarray(ed, dtype=np.int64).reshape(-1)
    out = {f: np.full(numQueries, -1, dtype=np.int32) for f in ("bestUnit", "bestDistance", "secondDistance")}
    hit = np.nonzero(ed >= 0)[0]
    key = (ed[hit] << 32) | hit
    order = np.lexsort((key, uq[hit]))                  # by query, then by key
    q, key = uq[hit][order], key[order]
    first = np.ones(len(q), dtype=bool)
    first[1:] = q[1:] != q[:-1]
    lead = np.nonzero(first)[0]
    out["bestUnit"][q[lead]] = key[lead] & 0xffffffff
    out["bestDistance"][q[lead]] = key[lead] >> 32
    has2 = lead + 1 < len(q)
    has2[has2] = q[lead[has2] + 1] == q[lead[has2]]
    out["secondDistance"][q[lead[has2]]] = key[lead[has2] + 1] >> 32
    return out


def cross_strands_model(fwd, rev):
    """The strand rule of a both-strand cross batch stated in numpy (what its cells must equal): fwd / rev are dictionaries
    of editDistance / numLocations / endLocation arrays of one shape, the cells of the queries and of their reverse
    complements.  The forward cell is reported where it is within k and not worse than the reverse one (ties go
    forward) and where neither is within k; the reverse cell elsewhere.  Returns (cells, strand): the three combined
    arrays, and uint8 strand bytes -- bit 0 the reverse complement is reported, bit 1 both strands reach the distance."""
    df, dr = (np.asarray(x["editDistance"]) for x in (fwd, rev))
    take_rev = (dr >= 0) & ((df < 0) | (dr < df))
    cells = {f: np.where(take_rev, np.asarray(rev[f]), np.asarray(fwd[f])).astype(np.int32)
             for f in ("editDistance", "numLocations", "endLocation")}
    strand = take_rev.astype(np.uint8) | (((df >= 0) & (df == dr)).astype(np.uint8) << 1)
    return cells, strand


def self_strands_model(fwd, rev):
    """The strand rule of a both-strand self batch stated in numpy (what its pairs must equal): fwd / rev are the
    condensed distances of seqs[i] and of reverse_complement(seqs[i]) against seqs[j], i < j.  Returns (ed, strand): the
    combined int32 distances and the uint8 strand bytes, by the rule of cross_strands_model()."""
    df, dr = np.asarray(fwd, dtype=np.int32), np.asarray(rev, dtype=np.int32)
    one, none = np.ones_like(df), np.full_like(df, -1)
    cells, strand = cross_strands_model({"editDistance": df, "numLocations": one, "endLocation": none},
                                        {"editDistance": dr, "numLocations": one, "endLocation": none})
    return cells["editDistance"], strand


def find_all(queries, target, k, additionalEqualities=None):
    """Every occurrence of every query within k edits along the target, in one device batch: the hits() arrays of
    SharedBatch(..., hits=True) -- the loop ``for q in queries: every window of target within k of q`` that adapter /
    primer trimming and multi-mapping searches run."""
    b = SharedBatch(queries, target, "HW", "distance", k, additionalEqualities, hits=True)
    try:
        b.run()
        return b.hits()
    finally:
        b.close()


def find_all_cross(queries, targets, k, additionalEqualities=None):
    """Every occurrence of every query within k edits along every target, in one device batch: the occurrences() arrays of
    CrossBatch(..., occurrences=True) -- find_all() over many targets (adapters or barcodes against a set of reads)."""
    b = CrossBatch(queries, targets, "HW", k, additionalEqualities, occurrences=True)
    try:
        b.run()
        return b.occurrences()
    finally:
        b.close()


def align_batch(queries, target, mode="HW", task="distance", k=-1, additionalEqualities=None, raw=False, strands="forward"):
    """[align(q, target, ...) for q in queries] in one device batch.  strands="both": every query is also searched as its
    reverse complement and the better strand is reported (ties: forward); the results gain the entries ``strand``
    (0 forward, 1 reverse complement) and ``bothStrands`` (1: the other strand reaches the same distance)."""
    if strands not in ("forward", "both"):
        raise ValueError("strands must be 'forward' or 'both'")
    both = strands == "both"
    b = (BothStrandsBatch if both else SharedBatch)(queries, target, mode, task, k, additionalEqualities)
    try:
        b.run()
        out = b.results(raw=raw)
        if both:
            st, bs = b.strands()
            for i, r in enumerate(out):
                r["strand"], r["bothStrands"] = int(st[i]), int(bs[i])
        return out
    finally:
        b.close()


def align_batch_oneshot(queries, target, targets=None, mode="HW", task="distance", k=-1, additionalEqualities=None):
    """The one-shot C entry points edlibAlignBatchSharedTarget / edlibAlignBatchPairs (pointer arrays in,
    EdlibAlignResult[] out; shards over EDLIB_AMD_DEVICES).  Returns raw result dicts."""
    L = lib()
    n = len(queries)
    cfg, keep = _make_config(mode, task, k, additionalEqualities)
    qs = [bytes(q) for q in queries]
    qarr = (C.c_char_p * max(n, 1))(*qs)
    qlen = (C.c_int * max(n, 1))(*[len(q) for q in qs])
    res = (AlignResult * max(n, 1))()
    if targets is None:
        rc = L.edlibAlignBatchSharedTarget(qarr, qlen, n, bytes(target), len(target), cfg, res)
    else:
        ts = [bytes(t) for t in targets]
        tarr = (C.c_char_p * max(n, 1))(*ts)
        tlen = (C.c_int * max(n, 1))(*[len(t) for t in ts])
        rc = L.edlibAlignBatchPairs(qarr, qlen, tarr, tlen, n, cfg, res)
    if rc != 0:
        raise RuntimeError("edlib_amd: one-shot batch failed: " + last_error())
    out = []
    for i in range(n):
        out.append(_raw_result(res[i]))
        L.edlibFreeAlignResult(res[i])
    return out


def align_pairs(queries, targets, mode="NW", task="distance", k=-1, additionalEqualities=None, raw=False):
    """[align(q, t, ...) for q, t in zip(queries, targets)] in one device batch."""
    b = PairBatch(queries, targets, mode, task, k, additionalEqualities)
    try:
        b.run()
        return b.results(raw=raw)
    finally:
        b.close()
