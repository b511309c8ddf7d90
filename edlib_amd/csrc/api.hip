// api.hip -- the C ABI: the five symbols of reference edlib.h plus the additive
// batch surface of include/edlib_amd.h.  No C++ types cross this boundary.
#define EDLIB_SHARED
#define EDLIB_BUILD
#include "engine_lanes.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <system_error>
#include <atomic>
#include <thread>
#include <vector>

using namespace edlib_amd;

// cross: a cross batch or a self batch (cross->isSelf()), windows: a window batch (impl unused by both)
struct EdlibAmdBatch { Batch impl; std::unique_ptr<CrossBatch> cross; std::unique_ptr<WindowBatch> windows; };

static int not_on_windows(EdlibAmdBatch* b, const char* what) {
    if (!b->windows) return 0;
    set_error("%s: not available on a window batch (edlibAmdBatchWindowView has its results)", what);
    return 1;
}

static int not_on_occurrences(EdlibAmdBatch* b, const char* what) {
    if (!b->cross || !b->cross->isOccurrences()) return 0;
    set_error("%s: not available on an occurrence batch (edlibAmdBatchCrossOccurrences has its results)", what);
    return 1;
}

static int not_on_self(EdlibAmdBatch* b, const char* what) {
    if (!b->cross || !b->cross->isSelf()) return 0;
    set_error("%s: not available on a self batch (edlibAmdBatchSelfView and edlibAmdBatchSelfHits have its results)", what);
    return 1;
}

static int not_on_cross(EdlibAmdBatch* b, const char* what) {
    if (not_on_windows(b, what) || not_on_self(b, what) || not_on_occurrences(b, what)) return 1;
    if (!b->cross) return 0;
    set_error("%s: not available on a cross batch (edlibAmdBatchCrossView has its results)", what);
    return 1;
}

static int not_on_hits(EdlibAmdBatch* b, const char* what) {
    if (b->cross || b->windows || !b->impl.isHits()) return 0;
    set_error("%s: not available on a hit-list read batch (edlibAmdBatchSharedHits has its results)", what);
    return 1;
}

static void fail_loudly(const char* where) {
    fprintf(stderr, "edlib (MI355X engine): %s failed: %s\n", where, last_error().c_str());
}

// No C++ exception may cross the C boundary (a caller written in C, or the reference's own clients, have no handler:
// std::bad_alloc out of a std::vector would be std::terminate).  Every entry point that can allocate runs inside this.
template <typename R, typename F>
static R guarded(const char* where, R failValue, F&& body) noexcept {
    try { return body(); }
    catch (const std::bad_alloc&) { try { set_error("%s: out of host memory", where); } catch (...) {} }
    catch (const std::exception& e) { try { set_error("%s: %s", where, e.what()); } catch (...) {} }
    catch (...) { try { set_error("%s: unknown C++ exception", where); } catch (...) {} }
    return failValue;
}

static EdlibAlignResult blank_result(int status) {
    EdlibAlignResult r;
    r.status = status; r.editDistance = -1;
    r.endLocations = nullptr; r.startLocations = nullptr; r.numLocations = 0;
    r.alignment = nullptr; r.alignmentLength = 0; r.alphabetLength = 0;
    return r;
}

// A batch whose init (a callable on the new batch) succeeded, or NULL with the error set
template <typename F>
static EdlibAmdBatch* create_batch(const char* where, F&& init) {
    EdlibAmdBatch* b = guarded(where, static_cast<EdlibAmdBatch*>(nullptr), [] { return new EdlibAmdBatch; });
    if (!b) return nullptr;
    if (guarded(where, 1, [&] { return init(*b); })) {
        delete b;
        return nullptr;
    }
    return b;
}

extern "C" {

// ---------------------------------------------------------------- edlib.h

// reference edlib.cpp:1465-1475
EDLIB_API EdlibAlignConfig edlibNewAlignConfig(int k, EdlibAlignMode mode, EdlibAlignTask task,
                                               const EdlibEqualityPair* additionalEqualities,
                                               int additionalEqualitiesLength) {
    EdlibAlignConfig c;
    c.k = k; c.mode = mode; c.task = task;
    c.additionalEqualities = additionalEqualities;
    c.additionalEqualitiesLength = additionalEqualitiesLength;
    return c;
}

// reference edlib.cpp:1477-1479
EDLIB_API EdlibAlignConfig edlibDefaultAlignConfig(void) {
    return edlibNewAlignConfig(-1, EDLIB_MODE_NW, EDLIB_TASK_DISTANCE, nullptr, 0);
}

// reference edlib.cpp:1481-1485
EDLIB_API void edlibFreeAlignResult(EdlibAlignResult result) {
    free(result.endLocations);
    free(result.startLocations);
    free(result.alignment);
}

// reference edlib.cpp:146-301: a batch of one.  No CPU fallback: if the device
// path cannot run the result carries EDLIB_STATUS_ERROR and a line goes to stderr.
EDLIB_API EdlibAlignResult edlibAlign(const char* query, int queryLength, const char* target,
                                      int targetLength, const EdlibAlignConfig config) {
    EdlibAlignResult r = blank_result(EDLIB_STATUS_OK);
    if (queryLength < 0 || targetLength < 0) { r.status = EDLIB_STATUS_ERROR; return r; }
    const int rc = guarded("edlibAlign", 1, [&] {
        const int f = align_one_fused(query, queryLength, target, targetLength, config, &r);     // small pairs: one launch
        return f == 2 ? align_one(query, queryLength, target, targetLength, config, &r) : f;
    });
    if (rc) {
        fail_loudly("edlibAlign");
        return blank_result(EDLIB_STATUS_ERROR);
    }
    return r;
}

// reference edlib.cpp:303-350: run-length encode EDLIB_EDOP_* codes.
EDLIB_API char* edlibAlignmentToCigar(const unsigned char* alignment, int alignmentLength,
                                      EdlibCigarFormat cigarFormat) {
    if (cigarFormat != EDLIB_CIGAR_EXTENDED && cigarFormat != EDLIB_CIGAR_STANDARD) return nullptr;
    static const char ext[4] = {'=', 'I', 'D', 'X'}, stdc[4] = {'M', 'I', 'D', 'M'};
    const char* letters = (cigarFormat == EDLIB_CIGAR_STANDARD) ? stdc : ext;
    return guarded("edlibAlignmentToCigar", static_cast<char*>(nullptr), [&]() -> char* {
        std::string out;
        int i = 0;
        while (i < alignmentLength) {
            if (alignment[i] > 3) return nullptr;
            const char c = letters[alignment[i]];
            int run = 0;
            while (i < alignmentLength && alignment[i] <= 3 && letters[alignment[i]] == c) { ++run; ++i; }
            out += std::to_string(run);
            out += c;
        }
        char* s = static_cast<char*>(malloc(out.size() + 1));
        if (s) memcpy(s, out.c_str(), out.size() + 1);
        return s;
    });
}

// ------------------------------------------------------------ edlib_amd.h

EDLIB_API int edlibAmdDeviceCount(void) { return device_count(); }
EDLIB_API const char* edlibAmdLastError(void) { return last_error().c_str(); }
EDLIB_API const char* edlibAmdVersion(void) { return "edlib-mi355x 0.1 (API of edlib 1.2.6)"; }

static EdlibAmdBatch* create_shared(const char* where, const char* queries, const long long* queryOffsets, int numQueries,
                                    const char* target, int targetLength, EdlibAlignConfig config, int device,
                                    bool bothStrands, bool hits) {
    if (targetLength < 0) { set_error("negative target length"); return nullptr; }
    const long long toff[2] = {0, targetLength};
    return create_batch(where, [&](EdlibAmdBatch& b) {
        return b.impl.init(queries, queryOffsets, numQueries, target, toff, 1, config, device, bothStrands, hits); });
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateShared(const char* queries, const long long* queryOffsets,
                                                   int numQueries, const char* target, int targetLength,
                                                   EdlibAlignConfig config, int device) {
    return create_shared("edlibAmdBatchCreateShared", queries, queryOffsets, numQueries, target, targetLength, config, device,
                         false, false);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreatePairs(const char* queries, const long long* queryOffsets,
                                                  const char* targets, const long long* targetOffsets,
                                                  int numPairs, EdlibAlignConfig config, int device) {
    // a one-pair batch is also a shared-target batch
    return create_batch("edlibAmdBatchCreatePairs", [&](EdlibAmdBatch& b) {
        return b.impl.init(queries, queryOffsets, numPairs, targets, targetOffsets, numPairs, config, device, false, false,
                           /*pairs=*/true); });
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSharedBothStrands(const char* queries, const long long* queryOffsets,
                                                              int numQueries, const char* target, int targetLength,
                                                              EdlibAlignConfig config, int device) {
    return create_shared("edlibAmdBatchCreateSharedBothStrands", queries, queryOffsets, numQueries, target, targetLength,
                         config, device, /*bothStrands=*/true, false);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSharedHits(const char* queries, const long long* queryOffsets, int numQueries,
                                                       const char* target, int targetLength, EdlibAlignConfig config,
                                                       int device) {
    return create_shared("edlibAmdBatchCreateSharedHits", queries, queryOffsets, numQueries, target, targetLength, config,
                         device, false, /*hits=*/true);
}

EDLIB_API int edlibAmdBatchSharedHits(EdlibAmdBatch* b, EdlibAmdReadHits* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_windows(b, "edlibAmdBatchSharedHits") || not_on_self(b, "edlibAmdBatchSharedHits")) return EDLIB_STATUS_ERROR;
    if (not_on_occurrences(b, "edlibAmdBatchSharedHits")) return EDLIB_STATUS_ERROR;
    if (b->cross) { set_error("edlibAmdBatchSharedHits: not a hit-list read batch (a cross batch has edlibAmdBatchCrossHits)"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchSharedHits", 1, [&] { return b->impl.hitsView(out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchStrandView(EdlibAmdBatch* b, EdlibAmdStrandView* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (b->cross && b->cross->bothStrands()) {
        set_error("edlibAmdBatchStrandView: not available on a cross batch (edlibAmdBatchCrossStrands has the strands of a "
                  "both-strand cross batch)");
        return EDLIB_STATUS_ERROR;
    }
    if (not_on_cross(b, "edlibAmdBatchStrandView") || not_on_hits(b, "edlibAmdBatchStrandView")) return EDLIB_STATUS_ERROR;
    return guarded("edlibAmdBatchStrandView", 1, [&] { return b->impl.strandView(out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API void edlibAmdReverseComplement(const char* in, int n, char* out) {
    for (int j = 0; j < n; ++j) out[j] = (char)complement_byte((uint8_t)in[n - 1 - j]);
}

static EdlibAmdBatch* create_cross(const char* where, const char* queries, const long long* queryOffsets, int numQueries,
                                   const char* targets, const long long* targetOffsets, int numTargets,
                                   EdlibAlignConfig config, int device, bool hits, bool strands = false,
                                   bool occurrences = false) {
    return create_batch(where, [&](EdlibAmdBatch& b) {
        b.cross.reset(new CrossBatch);
        return b.cross->init(queries, queryOffsets, numQueries, targets, targetOffsets, numTargets, config, device, hits,
                             strands, occurrences); });
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCross(const char* queries, const long long* queryOffsets, int numQueries,
                                                  const char* targets, const long long* targetOffsets, int numTargets,
                                                  EdlibAlignConfig config, int device) {
    return create_cross("edlibAmdBatchCreateCross", queries, queryOffsets, numQueries, targets, targetOffsets, numTargets,
                        config, device, false);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossHits(const char* queries, const long long* queryOffsets, int numQueries,
                                                      const char* targets, const long long* targetOffsets, int numTargets,
                                                      EdlibAlignConfig config, int device) {
    return create_cross("edlibAmdBatchCreateCrossHits", queries, queryOffsets, numQueries, targets, targetOffsets,
                        numTargets, config, device, true);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossBothStrands(const char* queries, const long long* queryOffsets,
                                                             int numQueries, const char* targets,
                                                             const long long* targetOffsets, int numTargets,
                                                             EdlibAlignConfig config, int device) {
    return create_cross("edlibAmdBatchCreateCrossBothStrands", queries, queryOffsets, numQueries, targets, targetOffsets,
                        numTargets, config, device, false, true);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossHitsBothStrands(const char* queries, const long long* queryOffsets,
                                                                 int numQueries, const char* targets,
                                                                 const long long* targetOffsets, int numTargets,
                                                                 EdlibAlignConfig config, int device) {
    return create_cross("edlibAmdBatchCreateCrossHitsBothStrands", queries, queryOffsets, numQueries, targets,
                        targetOffsets, numTargets, config, device, true, true);
}

EDLIB_API int edlibAmdBatchCrossStrands(EdlibAmdBatch* b, int what, EdlibAmdCrossStrands* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_windows(b, "edlibAmdBatchCrossStrands") || not_on_self(b, "edlibAmdBatchCrossStrands")) return EDLIB_STATUS_ERROR;
    if (!b->cross) {
        set_error("edlibAmdBatchCrossStrands: not a both-strand cross batch (a both-strand read batch has edlibAmdBatchStrandView)");
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchCrossStrands", 1, [&] { return b->cross->strandsView(what, out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchCrossView(EdlibAmdBatch* b, int what, EdlibAmdCrossView* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_windows(b, "edlibAmdBatchCrossView") || not_on_self(b, "edlibAmdBatchCrossView")) return EDLIB_STATUS_ERROR;
    if (!b->cross) { set_error("edlibAmdBatchCrossView: not a cross batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchCrossView", 1, [&] { return b->cross->view(what, out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchCrossHits(EdlibAmdBatch* b, EdlibAmdCrossHits* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_windows(b, "edlibAmdBatchCrossHits") || not_on_self(b, "edlibAmdBatchCrossHits")) return EDLIB_STATUS_ERROR;
    if (!b->cross) { set_error("edlibAmdBatchCrossHits: not a cross batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchCrossHits", 1, [&] { return b->cross->hitsView(out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossOccurrences(const char* queries, const long long* queryOffsets,
                                                             int numQueries, const char* targets,
                                                             const long long* targetOffsets, int numTargets,
                                                             EdlibAlignConfig config, int device) {
    return create_cross("edlibAmdBatchCreateCrossOccurrences", queries, queryOffsets, numQueries, targets, targetOffsets,
                        numTargets, config, device, /*hits=*/true, false, /*occurrences=*/true);
}

EDLIB_API int edlibAmdBatchCrossOccurrences(EdlibAmdBatch* b, EdlibAmdCrossOccurrences* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_windows(b, "edlibAmdBatchCrossOccurrences") || not_on_self(b, "edlibAmdBatchCrossOccurrences")) return EDLIB_STATUS_ERROR;
    if (!b->cross) {
        set_error("edlibAmdBatchCrossOccurrences: not an occurrence batch (create it with edlibAmdBatchCreateCrossOccurrences; "
                  "a hit-list read batch has edlibAmdBatchSharedHits)");
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchCrossOccurrences", 1, [&] { return b->cross->occurrencesView(out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchCrossSetTargets(EdlibAmdBatch* b, const char* targets, const long long* targetOffsets,
                                           int numTargets) {
    if (!b) { set_error("edlibAmdBatchCrossSetTargets: null batch"); return EDLIB_STATUS_ERROR; }
    if (not_on_windows(b, "edlibAmdBatchCrossSetTargets") || not_on_self(b, "edlibAmdBatchCrossSetTargets")) return EDLIB_STATUS_ERROR;
    if (!b->cross) {
        set_error("edlibAmdBatchCrossSetTargets: not a cross batch (only the targets of a cross batch can be replaced)");
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchCrossSetTargets", 1, [&] { return b->cross->setTargets(targets, targetOffsets, numTargets); })
               ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

static EdlibAmdBatch* create_self(const char* where, const char* seqs, const long long* offsets, int numSequences,
                                  EdlibAlignConfig config, int device, bool hits, bool strands = false) {
    return create_batch(where, [&](EdlibAmdBatch& b) {
        b.cross.reset(new CrossBatch);
        return b.cross->initSelf(seqs, offsets, numSequences, config, device, hits, strands); });
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelf(const char* seqs, const long long* offsets, int numSequences,
                                                 EdlibAlignConfig config, int device) {
    return create_self("edlibAmdBatchCreateSelf", seqs, offsets, numSequences, config, device, false);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfHits(const char* seqs, const long long* offsets, int numSequences,
                                                     EdlibAlignConfig config, int device) {
    return create_self("edlibAmdBatchCreateSelfHits", seqs, offsets, numSequences, config, device, true);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfHitsGrouped(const char* seqs, const long long* offsets, int numSequences,
                                                            const int* groups, EdlibAlignConfig config, int device) {
    return create_batch("edlibAmdBatchCreateSelfHitsGrouped", [&](EdlibAmdBatch& b) {
        b.cross.reset(new CrossBatch);
        return b.cross->initSelfGrouped(seqs, offsets, numSequences, groups, config, device); });
}

EDLIB_API int edlibAmdBatchSelfView(EdlibAmdBatch* b, int what, EdlibAmdSelfView* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_occurrences(b, "edlibAmdBatchSelfView")) return EDLIB_STATUS_ERROR;
    if (!b->cross || !b->cross->isSelf()) { set_error("edlibAmdBatchSelfView: not a self batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchSelfView", 1, [&] { return b->cross->selfView(what, out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchSelfHits(EdlibAmdBatch* b, EdlibAmdSelfHits* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_occurrences(b, "edlibAmdBatchSelfHits")) return EDLIB_STATUS_ERROR;
    if (!b->cross || !b->cross->isSelf()) { set_error("edlibAmdBatchSelfHits: not a self batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchSelfHits", 1, [&] { return b->cross->selfHitsView(out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfBothStrands(const char* seqs, const long long* offsets, int numSequences,
                                                            EdlibAlignConfig config, int device) {
    return create_self("edlibAmdBatchCreateSelfBothStrands", seqs, offsets, numSequences, config, device, false, true);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfHitsBothStrands(const char* seqs, const long long* offsets,
                                                                int numSequences, EdlibAlignConfig config, int device) {
    return create_self("edlibAmdBatchCreateSelfHitsBothStrands", seqs, offsets, numSequences, config, device, true, true);
}

EDLIB_API int edlibAmdBatchSelfStrands(EdlibAmdBatch* b, int what, EdlibAmdSelfStrands* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_occurrences(b, "edlibAmdBatchSelfStrands")) return EDLIB_STATUS_ERROR;
    if (!b->cross || !b->cross->isSelf()) { set_error("edlibAmdBatchSelfStrands: not a self batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchSelfStrands", 1, [&] { return b->cross->selfStrandsView(what, out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchSelfComponents(EdlibAmdBatch* b, int maxDistance, int what, EdlibAmdSelfComponents* out) {
    // (the parts first: they are judged without a batch)
    if (!what || (what & ~(EDLIB_AMD_COMPONENT_LABELS | EDLIB_AMD_COMPONENT_MEMBERS))) {
        set_error("edlibAmdBatchSelfComponents: unknown parts %d (EDLIB_AMD_COMPONENT_LABELS, with or without "
                  "EDLIB_AMD_COMPONENT_MEMBERS)", what);
        return EDLIB_STATUS_ERROR;
    }
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (!b->cross || !b->cross->isSelf()) {
        set_error("edlibAmdBatchSelfComponents: not a self batch (components are defined for self batches only: create one "
                  "with edlibAmdBatchCreateSelf or edlibAmdBatchCreateSelfHits)");
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchSelfComponents", 1, [&] { return b->cross->selfComponents(maxDistance, what, out); })
               ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

// (K first: it is judged without a batch)
static bool bad_neighbors_call(const char* fn, const EdlibAmdBatch* b, int K, const EdlibAmdNeighbors* out) {
    if (K < 1 || K > 64) { set_error("%s: K must be 1..64 (got %d)", fn, K); return true; }
    if (!b || !out) { set_error("%s: null argument", fn); return true; }
    return false;
}

EDLIB_API int edlibAmdBatchSelfNeighbors(EdlibAmdBatch* b, int K, int maxDistance, EdlibAmdNeighbors* out) {
    if (bad_neighbors_call("edlibAmdBatchSelfNeighbors", b, K, out)) return EDLIB_STATUS_ERROR;
    if (!b->cross || !b->cross->isSelf()) {
        set_error("edlibAmdBatchSelfNeighbors: not a self batch (create one with edlibAmdBatchCreateSelf or "
                  "edlibAmdBatchCreateSelfHits; a cross batch has edlibAmdBatchCrossNeighbors)");
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchSelfNeighbors", 1, [&] { return b->cross->selfNeighbors(K, maxDistance, out); })
               ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchCrossNeighbors(EdlibAmdBatch* b, int K, int maxDistance, EdlibAmdNeighbors* out) {
    if (bad_neighbors_call("edlibAmdBatchCrossNeighbors", b, K, out)) return EDLIB_STATUS_ERROR;
    if (!b->cross || b->cross->isSelf()) {
        set_error("edlibAmdBatchCrossNeighbors: not a cross batch (create one with edlibAmdBatchCreateCross or "
                  "edlibAmdBatchCreateCrossHits; a self batch has edlibAmdBatchSelfNeighbors)");
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchCrossNeighbors", 1, [&] { return b->cross->crossNeighbors(K, maxDistance, out); })
               ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

static EdlibAmdBatch* create_windows(const char* where, const char* queries, const long long* queryOffsets, int numQueries,
                                     const char* target, int targetLength, const int* unitQuery, const int* unitStart,
                                     const int* unitLength, const unsigned char* unitStrand, int numUnits,
                                     EdlibAlignConfig config, int device) {
    return create_batch(where, [&](EdlibAmdBatch& b) {
        b.windows.reset(new WindowBatch);
        return b.windows->init(queries, queryOffsets, numQueries, target, targetLength, unitQuery, unitStart, unitLength,
                               unitStrand, numUnits, config, device); });
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateWindows(const char* queries, const long long* queryOffsets, int numQueries,
                                                    const char* target, int targetLength, const int* unitQuery,
                                                    const int* unitStart, const int* unitLength, int numUnits,
                                                    EdlibAlignConfig config, int device) {
    return create_windows("edlibAmdBatchCreateWindows", queries, queryOffsets, numQueries, target, targetLength, unitQuery,
                          unitStart, unitLength, nullptr, numUnits, config, device);
}

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateWindowsStranded(const char* queries, const long long* queryOffsets,
                                                            int numQueries, const char* target, int targetLength,
                                                            const int* unitQuery, const int* unitStart,
                                                            const int* unitLength, const unsigned char* unitStrand,
                                                            int numUnits, EdlibAlignConfig config, int device) {
    return create_windows("edlibAmdBatchCreateWindowsStranded", queries, queryOffsets, numQueries, target, targetLength,
                          unitQuery, unitStart, unitLength, unitStrand, numUnits, config, device);
}

// "a cross batch", "a self batch", ...: the kind of a batch, for a refusal
static const char* kind_of(EdlibAmdBatch* b) {
    if (b->windows) return "a window batch";
    if (b->cross) return b->cross->isSelf() ? "a self batch" : b->cross->isOccurrences() ? "an occurrence batch" : "a cross batch";
    if (b->impl.isPairs()) return "a pair batch";
    return b->impl.isHits() ? "a hit-list read batch" : b->impl.isBothStrands() ? "a both-strand read batch" : "a shared-target read batch";
}

EDLIB_API int edlibAmdBatchPairsSetPairs(EdlibAmdBatch* b, const char* queries, const long long* queryOffsets,
                                         const char* targets, const long long* targetOffsets, int numPairs) {
    if (!b) { set_error("edlibAmdBatchPairsSetPairs: null batch"); return EDLIB_STATUS_ERROR; }
    if (b->windows || b->cross || !b->impl.isPairs()) {
        set_error("edlibAmdBatchPairsSetPairs: not available on %s (only the pairs of a batch made by edlibAmdBatchCreatePairs "
                  "can be replaced)", kind_of(b));
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchPairsSetPairs", 1, [&] {
               return b->impl.setPairs(queries, queryOffsets, targets, targetOffsets, numPairs); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchPairsSetWindows(EdlibAmdBatch* pairs, EdlibAmdBatch* windows, const int* pairQuery,
                                           const int* pairStart, const int* pairLength, const unsigned char* pairStrand,
                                           int numPairs) {
    static const char* const fn = "edlibAmdBatchPairsSetWindows";
    if (!pairs || !windows) {                     // (both handles before either is read)
        set_error("%s: %s%s%s", fn, pairs ? "" : "null pair batch", !pairs && !windows ? " and " : "",
                  windows ? "" : "null window batch");
        return EDLIB_STATUS_ERROR;
    }
    if (pairs->windows || pairs->cross || !pairs->impl.isPairs()) {
        set_error("%s: not available on %s (only the pairs of a batch made by edlibAmdBatchCreatePairs can be replaced)", fn,
                  kind_of(pairs));
        return EDLIB_STATUS_ERROR;
    }
    if (!windows->windows) {
        set_error("%s: the pairs cannot be gathered from %s (only from a window batch)", fn, kind_of(windows));
        return EDLIB_STATUS_ERROR;
    }
    if (pairs->impl.device() != windows->windows->device()) {
        set_error("%s: the pair batch is on device %d and the window batch on device %d: the gather does not cross devices", fn,
                  pairs->impl.device(), windows->windows->device());
        return EDLIB_STATUS_ERROR;
    }
    return guarded(fn, 1, [&] {
               WindowSource src;
               if (windows->windows->gatherSource(fn, src)) return 1;
               return pairs->impl.setWindows(fn, src, pairQuery, pairStart, pairLength, pairStrand, numPairs);
           }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchPairsSetSharedWindows(EdlibAmdBatch* pairs, EdlibAmdBatch* reads, const int* pairQuery,
                                                 const int* pairStart, const int* pairLength,
                                                 const unsigned char* pairStrand, int numPairs) {
    static const char* const fn = "edlibAmdBatchPairsSetSharedWindows";
    if (!pairs || !reads) {                       // (both handles before either is read)
        set_error("%s: %s%s%s", fn, pairs ? "" : "null pair batch", !pairs && !reads ? " and " : "",
                  reads ? "" : "null read batch");
        return EDLIB_STATUS_ERROR;
    }
    if (pairs->windows || pairs->cross || !pairs->impl.isPairs()) {
        set_error("%s: not available on %s (only the pairs of a batch made by edlibAmdBatchCreatePairs can be replaced)", fn,
                  kind_of(pairs));
        return EDLIB_STATUS_ERROR;
    }
    if (reads->windows || reads->cross || reads->impl.isPairs()) {
        set_error("%s: the pairs cannot be gathered from %s (only from a read batch: edlibAmdBatchCreateShared, "
                  "...SharedBothStrands or ...SharedHits; a window batch has edlibAmdBatchPairsSetWindows)", fn, kind_of(reads));
        return EDLIB_STATUS_ERROR;
    }
    if (pairs->impl.device() != reads->impl.device()) {
        set_error("%s: the pair batch is on device %d and the read batch on device %d: the gather does not cross devices", fn,
                  pairs->impl.device(), reads->impl.device());
        return EDLIB_STATUS_ERROR;
    }
    return guarded(fn, 1, [&] {
               // (gatherSource waits for the read batch's stream -- its Create uploads asynchronously -- and changes nothing
               // a caller can observe; the tuples and the envelope are then judged before the pair batch changes)
               WindowSource src;
               if (reads->impl.gatherSource(fn, src)) return 1;
               return pairs->impl.setWindows(fn, src, pairQuery, pairStart, pairLength, pairStrand, numPairs);
           }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchPairsSetCells(EdlibAmdBatch* pairs, EdlibAmdBatch* cross, const int* pairQuery,
                                         const int* pairTarget, const int* pairStart, const int* pairLength,
                                         const unsigned char* pairStrand, int numPairs) {
    static const char* const fn = "edlibAmdBatchPairsSetCells";
    if (!pairs || !cross) {                       // (both handles before either is read)
        set_error("%s: %s%s%s", fn, pairs ? "" : "null pair batch", !pairs && !cross ? " and " : "",
                  cross ? "" : "null cross batch");
        return EDLIB_STATUS_ERROR;
    }
    if (pairs->windows || pairs->cross || !pairs->impl.isPairs()) {
        set_error("%s: not available on %s (only the pairs of a batch made by edlibAmdBatchCreatePairs can be replaced)", fn,
                  kind_of(pairs));
        return EDLIB_STATUS_ERROR;
    }
    if (!cross->cross) {
        set_error("%s: the pairs cannot be gathered from %s (only from a cross, occurrence or self batch; a window batch has "
                  "edlibAmdBatchPairsSetWindows, a read batch edlibAmdBatchPairsSetSharedWindows)", fn, kind_of(cross));
        return EDLIB_STATUS_ERROR;
    }
    if (pairs->impl.device() != cross->cross->device()) {
        set_error("%s: the pair batch is on device %d and %s on device %d: the gather does not cross devices", fn,
                  pairs->impl.device(), kind_of(cross), cross->cross->device());
        return EDLIB_STATUS_ERROR;
    }
    return guarded(fn, 1, [&] {
               // (gatherSource waits for the source's stream -- its Create and SetTargets prepare asynchronously -- and
               // changes nothing a caller can observe; the tuples and the envelope are then judged before the pair batch changes)
               CellSource src;
               if (cross->cross->gatherSource(fn, src)) return 1;
               return pairs->impl.setCells(fn, src, pairQuery, pairTarget, pairStart, pairLength, pairStrand, numPairs);
           }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchWindowsSetUnits(EdlibAmdBatch* b, const char* queries, const long long* queryOffsets,
                                           int numQueries, const int* unitQuery, const int* unitStart,
                                           const int* unitLength, const unsigned char* unitStrand, int numUnits) {
    if (!b) { set_error("edlibAmdBatchWindowsSetUnits: null batch"); return EDLIB_STATUS_ERROR; }
    if (!b->windows) {
        set_error("edlibAmdBatchWindowsSetUnits: not available on %s (only the queries and units of a window batch can be "
                  "replaced)", kind_of(b));
        return EDLIB_STATUS_ERROR;
    }
    return guarded("edlibAmdBatchWindowsSetUnits", 1, [&] {
               return b->windows->setUnits(queries, queryOffsets, numQueries, unitQuery, unitStart, unitLength, unitStrand,
                                           numUnits); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchWindowView(EdlibAmdBatch* b, int what, EdlibAmdWindowView* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_self(b, "edlibAmdBatchWindowView") || not_on_occurrences(b, "edlibAmdBatchWindowView")) return EDLIB_STATUS_ERROR;
    if (!b->windows) { set_error("edlibAmdBatchWindowView: not a window batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchWindowView", 1, [&] { return b->windows->view(what, out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchRun(EdlibAmdBatch* b) {
    if (!b) { set_error("null batch"); return EDLIB_STATUS_ERROR; }
    return guarded("edlibAmdBatchRun", 1, [&] {
               return b->windows ? b->windows->run() : b->cross ? b->cross->run() : b->impl.run(); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchResults(EdlibAmdBatch* b, EdlibAlignResult* results) {
    if (!b || !results) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_cross(b, "edlibAmdBatchResults") || not_on_hits(b, "edlibAmdBatchResults")) return EDLIB_STATUS_ERROR;
    return guarded("edlibAmdBatchResults", 1, [&] { return b->impl.results(results); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchResultsFlat(EdlibAmdBatch* b, int* status, int* editDistance, int* numLocations,
                                       int* alphabetLength, long long* locOffsets, int** endLocations,
                                       int** startLocations, long long* alnOffsets, unsigned char** alignment) {
    if (!b) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_cross(b, "edlibAmdBatchResultsFlat") || not_on_hits(b, "edlibAmdBatchResultsFlat")) return EDLIB_STATUS_ERROR;
    return guarded("edlibAmdBatchResultsFlat", 1, [&] {
               return b->impl.resultsFlat(status, editDistance, numLocations, alphabetLength, locOffsets, endLocations,
                                          startLocations, alnOffsets, alignment); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchResultsView(EdlibAmdBatch* b, EdlibAmdResultsView* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_cross(b, "edlibAmdBatchResultsView") || not_on_hits(b, "edlibAmdBatchResultsView")) return EDLIB_STATUS_ERROR;
    return guarded("edlibAmdBatchResultsView", 1, [&] { return b->impl.resultsView(out); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API int edlibAmdBatchCigarView(EdlibAmdBatch* b, EdlibCigarFormat cigarFormat, const char** chars, const long long** offsets) {
    if (!b) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (not_on_cross(b, "edlibAmdBatchCigarView") || not_on_hits(b, "edlibAmdBatchCigarView")) return EDLIB_STATUS_ERROR;
    return guarded("edlibAmdBatchCigarView", 1, [&] { return b->impl.cigarView((int)cigarFormat, chars, offsets); }) ? EDLIB_STATUS_ERROR : EDLIB_STATUS_OK;
}

EDLIB_API void edlibAmdFreeResults(EdlibAlignResult* results, int n) {
    if (!results) return;
    for (int i = 0; i < n; ++i) {
        edlibFreeAlignResult(results[i]);
        results[i].endLocations = nullptr; results[i].startLocations = nullptr; results[i].alignment = nullptr;
    }
}

EDLIB_API void edlibAmdTrim(void) { (void)guarded("edlibAmdTrim", 0, [] { pool_trim(); return 0; }); }

EDLIB_API int edlibAmdBatchStats(EdlibAmdBatch* b, EdlibAmdBatchStats* out) {
    if (!b || !out) { set_error("null argument"); return EDLIB_STATUS_ERROR; }
    if (b->windows) { *out = b->windows->stats; return EDLIB_STATUS_OK; }
    if (b->cross) { *out = b->cross->stats; return EDLIB_STATUS_OK; }
    (void)guarded("edlibAmdBatchStats", 0, [&] { b->impl.finishStats(); return 0; });
    *out = b->impl.stats;
    return EDLIB_STATUS_OK;
}

EDLIB_API void edlibAmdBatchDestroy(EdlibAmdBatch* b) { delete b; }

// The sequences of a one-shot call, packed back to back.  The pack goes straight into pinned staging (cached by the
// library) so that the upload that follows runs at link rate with no second host copy, and large packs are cut over
// a few host threads (1M x 150 bp = 150 MB of 150-byte memcpy: ~35 ms on one thread).
struct Packed {
    PinBuf pin; std::vector<char> small; std::vector<long long> off;
    const char* data() const { return pin.p ? reinterpret_cast<const char*>(pin.p) : small.data(); }
};

// false if a length is negative (edlibAlign answers EDLIB_STATUS_ERROR for those: so does the batch)
static bool pack(const char* const* seqs, const int* lens, int n, Packed& out) {
    out.off.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (lens[i] < 0) { set_error("negative sequence length at index %d", i); return false; }
        out.off[i + 1] = out.off[i] + lens[i];
    }
    const size_t bytes = (size_t)out.off[n] + 1;
    char* dst;
    if (bytes >= (1u << 20) && device_count() > 0 && out.pin.alloc(bytes) == hipSuccess) dst = reinterpret_cast<char*>(out.pin.p);
    else { (void)hipGetLastError(); out.pin.release(); out.small.resize(bytes); dst = out.small.data(); }
    auto copy = [&](int lo, int hi) { for (int i = lo; i < hi; ++i) if (lens[i] > 0) memcpy(dst + out.off[i], seqs[i], (size_t)lens[i]); };
    const int nthreads = bytes >= (32u << 20) ? host_threads(6) : 1;
    int done = 0;
    if (nthreads > 1) {
        std::vector<std::thread> th;
        th.reserve(nthreads);
        ThreadJoiner join(th);
        try {
            for (int t = 0; t < nthreads; ++t) {
                const int hi = (int)((long long)n * (t + 1) / nthreads);
                th.emplace_back(copy, done, hi);
                done = hi;
            }
        } catch (const std::system_error&) {}          // thread limit: this thread copies the rest
    }
    if (done < n) copy(done, n);
    return true;
}

// Devices the one-shot batch entry points shard over (contiguous slices of the units,
// target replicated, one host thread + one stream per device, no collective).  Default: device 0.
// EDLIB_AMD_DEVICES=all | "0,1,2,..." (a device may be listed twice: used by the tests on a 1-GPU box).
static std::vector<int> oneshot_devices() {
    std::vector<int> devs;
    const char* env = getenv("EDLIB_AMD_DEVICES");
    const int ndev = device_count();
    if (env && !strcmp(env, "all")) { for (int d = 0; d < ndev; ++d) devs.push_back(d); }
    else if (env && *env) {
        for (const char* p = env; *p;) {
            char* e; const long d = strtol(p, &e, 10);
            if (e == p) break;
            if (d >= 0 && d < ndev) devs.push_back((int)d);
            p = (*e == ',') ? e + 1 : e;
        }
    }
    if (devs.empty()) devs.push_back(default_device());
    return devs;
}

// Runs units [lo, hi) of a packed batch on one device.  toff == nullptr: shared target.
static int run_shard(const char* q, const long long* qoff, const char* t, const long long* toff, int targetLength,
                     int lo, int hi, EdlibAlignConfig config, int device, EdlibAlignResult* results, std::string* err) {
    EdlibAmdBatch* b = toff ? edlibAmdBatchCreatePairs(q, qoff + lo, t, toff + lo, hi - lo, config, device)
                            : edlibAmdBatchCreateShared(q, qoff + lo, hi - lo, t, targetLength, config, device);
    int rc = b ? edlibAmdBatchRun(b) : EDLIB_STATUS_ERROR;
    if (rc == EDLIB_STATUS_OK) rc = edlibAmdBatchResults(b, results + lo);
    if (rc != EDLIB_STATUS_OK) *err = last_error();
    if (b) edlibAmdBatchDestroy(b);
    return rc;
}

static int run_sharded(const char* q, const long long* qoff, const char* t, const long long* toff, int targetLength,
                       int n, EdlibAlignConfig config, EdlibAlignResult* results, const char* where) {
    const std::vector<int> devs = oneshot_devices();
    const int world = (int)std::min<size_t>(devs.size(), (size_t)std::max(1, n));
    std::vector<int> rc(world, EDLIB_STATUS_OK);
    std::vector<std::string> err(world);
    const int per = (n + world - 1) / world;                     // same rule as edlib_amd/parallel.py
    // Independent PAIRS vary in work (query x target cells): static slices leave devices idle behind the one that drew the
    // long pairs.  SURVEY.md 8e: a shared queue of chunks of about equal work (contiguous unit ranges, ~8 per device, cut
    // where the running sum of qlen * tlen crosses the next multiple of total / chunks) that the device threads pull from
    // with one atomic counter.  Shared-target read batches (equal reads) and EDLIB_AMD_SHARD=static keep the static slices.
    std::vector<int> cuts;                                       // chunk c = units [cuts[c], cuts[c + 1])
    {
        const char* how = getenv("EDLIB_AMD_SHARD");
        const bool queue = toff != nullptr && world > 1 && n >= 2 * world && !(how && !strcmp(how, "static"));
        if (queue) {
            double total = 0;
            for (int i = 0; i < n; ++i) total += (double)(qoff[i + 1] - qoff[i] + 1) * (double)(toff[i + 1] - toff[i] + 1);
            const int chunks = std::min(n, 8 * world);
            double acc = 0; int next = 1;
            cuts.push_back(0);
            for (int i = 0; i < n; ++i) {
                acc += (double)(qoff[i + 1] - qoff[i] + 1) * (double)(toff[i + 1] - toff[i] + 1);
                if (acc >= total * next / chunks && i + 1 < n) { cuts.push_back(i + 1); while (acc >= total * next / chunks) ++next; }
            }
            cuts.push_back(n);
        }
    }
    std::atomic<int> nextChunk{0};
    auto work = [&](int r) {                                     // a thread body: nothing may escape it
        rc[r] = guarded(where, (int)EDLIB_STATUS_ERROR, [&] {
            if (!cuts.empty()) {
                for (;;) {
                    const int c = nextChunk.fetch_add(1);
                    if (c + 1 >= (int)cuts.size()) return (int)EDLIB_STATUS_OK;
                    const int st = run_shard(q, qoff, t, toff, targetLength, cuts[c], cuts[c + 1], config, devs[r], results, &err[r]);
                    if (st != EDLIB_STATUS_OK) { nextChunk.store((int)cuts.size()); return st; }       // nobody starts another chunk
                }
            }
            const int lo = std::min(n, r * per), hi = std::min(n, lo + per);
            return (hi > lo || n == 0) ? run_shard(q, qoff, t, toff, targetLength, lo, hi, config, devs[r], results, &err[r])
                                       : (int)EDLIB_STATUS_OK;
        });
    };
    if (world == 1) work(0);
    else {
        std::vector<std::thread> th;
        th.reserve(world);
        int started = 0;
        {
            ThreadJoiner join(th);
            try { for (; started < world; ++started) th.emplace_back(work, started); }
            catch (const std::system_error&) {}        // thread limit: the shards without a thread run here, one by one
            for (int r = started; r < world; ++r) work(r);
        }
    }
    for (int r = 0; r < world; ++r) {
        if (rc[r] == EDLIB_STATUS_OK) continue;
        set_error("%s", err[r].c_str());
        fail_loudly(where);
        for (int i = 0; i < n; ++i) {                            // all or nothing: free what other shards produced
            if (results[i].status == EDLIB_STATUS_OK) edlibFreeAlignResult(results[i]);
            results[i] = blank_result(EDLIB_STATUS_ERROR);
        }
        return EDLIB_STATUS_ERROR;
    }
    return EDLIB_STATUS_OK;
}

EDLIB_API int edlibAlignBatchSharedTarget(const char* const* queries, const int* queryLengths, int numQueries,
                                          const char* target, int targetLength, EdlibAlignConfig config,
                                          EdlibAlignResult* results) {
    if (numQueries < 0 || targetLength < 0) { set_error("negative size"); return EDLIB_STATUS_ERROR; }
    for (int i = 0; i < numQueries; ++i) results[i] = blank_result(EDLIB_STATUS_ERROR);
    return guarded("edlibAlignBatchSharedTarget", (int)EDLIB_STATUS_ERROR, [&] {
        Packed q;
        if (!pack(queries, queryLengths, numQueries, q)) return (int)EDLIB_STATUS_ERROR;
        return run_sharded(q.data(), q.off.data(), target, nullptr, targetLength, numQueries, config, results,
                           "edlibAlignBatchSharedTarget");
    });
}

EDLIB_API int edlibAlignBatchPairs(const char* const* queries, const int* queryLengths,
                                   const char* const* targets, const int* targetLengths, int numPairs,
                                   EdlibAlignConfig config, EdlibAlignResult* results) {
    if (numPairs < 0) { set_error("negative size"); return EDLIB_STATUS_ERROR; }
    for (int i = 0; i < numPairs; ++i) results[i] = blank_result(EDLIB_STATUS_ERROR);
    return guarded("edlibAlignBatchPairs", (int)EDLIB_STATUS_ERROR, [&] {
        Packed q, t;
        if (!pack(queries, queryLengths, numPairs, q) || !pack(targets, targetLengths, numPairs, t)) return (int)EDLIB_STATUS_ERROR;
        return run_sharded(q.data(), q.off.data(), t.data(), t.off.data(), 0, numPairs, config, results,
                           "edlibAlignBatchPairs");
    });
}

}  // extern "C"
