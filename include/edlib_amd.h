/*
 * edlib_amd.h -- additive batch surface of the MI355X edit-distance engine.
 *
 * edlib.h (the reference's five symbols) stays untouched; everything here is
 * new.  The natural batching site in the reference is the per-query loop of
 * its CLI (apps/aligner/aligner.cpp:162-225: one edlibAlign() per query
 * against the same target) and, for pairwise work, any caller that loops over
 * edlibAlign() (bindings/python/edlib.pyx:128-129).  These entry points take
 * the whole loop at once so the GPU sees a batch.
 *
 * All functions are plain C ABI: pointers + sizes, no C++ or torch types.
 * Return value: EDLIB_STATUS_OK (0) / EDLIB_STATUS_ERROR (1) unless stated;
 * edlibAmdLastError() gives the reason.  There is no CPU fallback: without a
 * usable HIP device every compute entry point fails with EDLIB_STATUS_ERROR.
 */
#ifndef EDLIB_AMD_H
#define EDLIB_AMD_H

#include "edlib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- process */

/* Number of usable HIP devices (0 when the runtime or a device is missing). */
EDLIB_API int edlibAmdDeviceCount(void);
/* Message of the last failing call on this thread ("" if none). */
EDLIB_API const char* edlibAmdLastError(void);
EDLIB_API const char* edlibAmdVersion(void);

/* ------------------------------------------------------- one-shot batches */

/* numQueries queries against ONE target: replaces the loop
 * `for q: results[q] = edlibAlign(queries[q], .., target, .., config)`
 * (apps/aligner/aligner.cpp:162-172).  results[] must hold numQueries
 * entries; each is exactly what edlibAlign() would have returned and is
 * released the same way (edlibFreeAlignResult / free).
 * Environment: EDLIB_AMD_DEVICES = "all" or a comma list of device ordinals
 * shards the units over several GPUs of the node (contiguous slices, target
 * replicated, one host thread + stream per device, no collective); default
 * is EDLIB_AMD_DEVICE if set, else the calling thread's current HIP device.  All-or-nothing: if any shard fails every result is ERROR. */
EDLIB_API int edlibAlignBatchSharedTarget(
    const char* const* queries, const int* queryLengths, int numQueries,
    const char* target, int targetLength,
    EdlibAlignConfig config, EdlibAlignResult* results);

/* numPairs independent (query, target) pairs: replaces
 * `for i: results[i] = edlibAlign(queries[i], .., targets[i], .., config)`. */
EDLIB_API int edlibAlignBatchPairs(
    const char* const* queries, const int* queryLengths,
    const char* const* targets, const int* targetLengths, int numPairs,
    EdlibAlignConfig config, EdlibAlignResult* results);

/* ------------------------------------------- resident batches (sessions) */
/* Upload once, run many times with everything resident in HBM; this is what
 * bench.py times.  Sequences are passed packed: `queries` is the
 * concatenation of all query bytes and queryOffsets[i]..queryOffsets[i+1]
 * delimits query i (numQueries+1 offsets). */

typedef struct EdlibAmdBatch EdlibAmdBatch;

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateShared(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* target, int targetLength,
    EdlibAlignConfig config, int device);

EDLIB_API EdlibAmdBatch* edlibAmdBatchCreatePairs(
    const char* queries, const long long* queryOffsets,
    const char* targets, const long long* targetOffsets, int numPairs,
    EdlibAlignConfig config, int device);

/* numQueries queries against numTargets targets, every pair (a cross batch): replaces
 * `for t: for q: d[t][q] = edlibAlign(queries[q], .., targets[t], .., config).editDistance`
 * (barcode / primer demultiplexing, all-against-all distance matrices, reads against several contigs) without
 * replicating a byte per cell.  config.task must be EDLIB_TASK_DISTANCE (otherwise NULL; align the chosen pairs
 * with a pair batch for locations or paths); NW, SHW and HW, any k, additionalEqualities.  Cells of queries up to
 * 256 bases and targets up to 65,536 bases over at most 16 target symbols (all targets together) run on the cross
 * kernel; every other target runs through the shared-target engine over all queries (one internal session per
 * such target: right for long contigs, slow for thousands of short targets over a wide alphabet), and longer
 * queries against the remaining targets through one internal pair batch.
 * Run, Stats and Destroy work as for the other batches (Stats.path bit 3: the cross kernel; Stats.cells the sum of
 * queryLength * targetLength over all cells); Results, ResultsFlat, ResultsView and CigarView fail. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCross(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* targets, const long long* targetOffsets, int numTargets,
    EdlibAlignConfig config, int device);

/* out[j] = C[in[n-1-j]]: the reverse complement of a nucleotide sequence.  C swaps A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H,
 * sends U to A, and leaves S, W, N and every other byte as they are; lower case likewise (u -> a).  in and out must not
 * overlap.  Host only, needs no device. */
EDLIB_API void edlibAmdReverseComplement(const char* in, int n, char* out);

/* As edlibAmdBatchCreateShared, but every query is searched on both strands: as itself and as its reverse complement
 * (edlibAmdReverseComplement), which the library makes on the device.  With d+ / d- the two edit distances (-1: nothing
 * within k), unit i reports
 *   d+ >= 0 and (d- < 0 or d+ <= d-):  the forward result, every field; strand 0; bothStrands 1 iff d- == d+
 *   otherwise, d- >= 0:                the result of the reverse complement, every field; strand 1; bothStrands 0
 *   d+ == d- == -1:                    the forward result (distance -1, no locations); strand 0; bothStrands 0
 * Ties go to the forward strand.  For strand 1 the locations are target coordinates of the alignment of the reverse
 * complement, and the alignment's query is the reverse complement.  All modes and tasks, any k, additionalEqualities.
 * Run / Results / ResultsFlat / ResultsView / CigarView / Stats / Destroy work as for a shared batch and report numQueries
 * units; Stats.cells counts both strands.  Reads of up to 256 bases in HW mode (the read groups) stop climbing the
 * threshold levels as soon as one strand has resolved: a batch whose reads each match on one strand costs about two
 * single-strand steps, not the full-height scan of every wrong strand. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSharedBothStrands(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* target, int targetLength,
    EdlibAlignConfig config, int device);

/* Which strand every unit of the last Run of a both-strand batch reports.  Pinned memory the batch owns, valid until the
 * next Run / Destroy; fails on any other kind of batch. */
typedef struct {
    int numUnits;
    const unsigned char* strand;        /* [numUnits] 0 forward, 1 reverse complement                  */
    const unsigned char* bothStrands;   /* [numUnits] 1: the other strand reaches the same distance    */
} EdlibAmdStrandView;
EDLIB_API int edlibAmdBatchStrandView(EdlibAmdBatch* batch, EdlibAmdStrandView* out);

/* One pass of the device path over the resident batch (encode target, build
 * the query profiles, scan, merge; for LOC/PATH also start locations and
 * traceback), then wait for it.  Results stay on the device. */
EDLIB_API int edlibAmdBatchRun(EdlibAmdBatch* batch);

/* Copy the results of the last Run to the host as EdlibAlignResult[numQueries]
 * (malloc'd arrays, caller frees each with edlibFreeAlignResult).  On failure (EDLIB_STATUS_ERROR, e.g. host
 * memory exhausted) every entry is blank with status EDLIB_STATUS_ERROR: nothing is left for the caller to free.
 * No entry point of this library lets a C++ exception out. */
EDLIB_API int edlibAmdBatchResults(EdlibAmdBatch* batch, EdlibAlignResult* results);

/* The same results as flat arrays: no per-unit malloc, one array per field (what a numpy / columnar caller
 * wants).  status, editDistance, numLocations, alphabetLength: caller-provided int[numQueries];
 * locOffsets, alnOffsets: caller-provided long long[numQueries + 1]; *endLocations, *startLocations
 * (locOffsets[numQueries] ints; startLocations is NULL unless the task produced start locations) and
 * *alignment (alnOffsets[numQueries] op bytes) are malloc'd, the caller free()s them.  Any pointer may be NULL. */
EDLIB_API int edlibAmdBatchResultsFlat(EdlibAmdBatch* batch, int* status, int* editDistance, int* numLocations,
                                       int* alphabetLength, long long* locOffsets, int** endLocations,
                                       int** startLocations, long long* alnOffsets, unsigned char** alignment);

/* The same arrays WITHOUT copies: pointers into pinned host memory the batch owns, valid until the next Run / Destroy of
 * this batch.  For a batch of short pairs ("flat": every unit a pair of at most 16 blocks) the arrays are laid out by
 * device kernels -- the k filter, the -1 location of the padded last block, start locations, the dense op bytes, their
 * offsets by a prefix sum -- and arrive as one block at link rate; other batches build them once on the host.
 * startLocations is NULL unless the task produced start locations, alignment NULL unless it produced paths. */
typedef struct {
    int numUnits;
    const int* status;              /* [numUnits] EDLIB_STATUS_*                                  */
    const int* editDistance;        /* [numUnits] -1: no alignment within k                       */
    const int* numLocations;        /* [numUnits]                                                 */
    const int* alphabetLength;      /* [numUnits]                                                 */
    const long long* locOffsets;    /* [numUnits + 1] into endLocations / startLocations          */
    const int* endLocations;
    const int* startLocations;
    const long long* alnOffsets;    /* [numUnits + 1] into alignment (EDLIB_EDOP_* bytes)         */
    const unsigned char* alignment;
} EdlibAmdResultsView;
EDLIB_API int edlibAmdBatchResultsView(EdlibAmdBatch* batch, EdlibAmdResultsView* out);

/* edlibAlignmentToCigar() over every op string of the last Run (a TASK_PATH batch): *chars = the NUL-terminated CIGAR
 * strings one after the other, (*offsets)[i] = where string i starts ((*offsets)[numUnits] = all bytes); a unit without
 * an alignment has the empty string.  Same lifetime as the view.  Flat batches: made on the device. */
EDLIB_API int edlibAmdBatchCigarView(EdlibAmdBatch* batch, EdlibCigarFormat cigarFormat,
                                     const char** chars, const long long** offsets);

/* Results of the last Run of a cross batch, as pointers into pinned host memory the batch owns (valid until the next
 * Run / Destroy).  Only the parts asked for in `what` (EDLIB_AMD_CROSS_MATRIX | EDLIB_AMD_CROSS_BEST) cross the link;
 * the others are NULL.  Cell (q, t) of the matrix is at [t * numQueries + q] and equals edlibAlign(query q, target t,
 * config) in editDistance (-1: above k), numLocations and the first end location (-1 when there is none).
 * Best hits: per target over the queries and per query over the targets, the lowest index wins a tie; the second
 * distance is the smallest over the other indices (equal to the best on a tie); -1 where no cell is within k. */
typedef struct {
    int numQueries, numTargets;
    const int* editDistance;          /* [numTargets * numQueries]                                  */
    const int* numLocations;          /* [numTargets * numQueries]                                  */
    const int* endLocation;           /* [numTargets * numQueries] endLocations[0], else -1         */
    const int* bestQuery;             /* [numTargets]                                               */
    const int* bestQueryDistance;     /* [numTargets]                                               */
    const int* secondQueryDistance;   /* [numTargets]                                               */
    const int* bestTarget;            /* [numQueries]                                               */
    const int* bestTargetDistance;    /* [numQueries]                                               */
    const int* secondTargetDistance;  /* [numQueries]                                               */
} EdlibAmdCrossView;
#define EDLIB_AMD_CROSS_MATRIX 1
#define EDLIB_AMD_CROSS_BEST   2
EDLIB_API int edlibAmdBatchCrossView(EdlibAmdBatch* batch, int what, EdlibAmdCrossView* out);

/* A cross batch whose results are the cells within k as a list, without a numQueries x numTargets matrix anywhere
 * (device or host).  Same inputs, routing, modes and additionalEqualities as edlibAmdBatchCreateCross; config.task
 * must be EDLIB_TASK_DISTANCE and config.k >= 0 (otherwise NULL, with the reason in edlibAmdLastError()).
 * Run, Stats and Destroy work as for a dense cross batch; edlibAmdBatchCrossView gives EDLIB_AMD_CROSS_BEST (equal to
 * a dense batch's) and refuses EDLIB_AMD_CROSS_MATRIX; Results, ResultsFlat, ResultsView and CigarView fail.
 * The device list starts at max(2^20, numQueries + numTargets) hits; a Run that finds more grows it to its count and
 * scans once more (later Runs of the batch fit); a list that does not fit in device memory fails the Run with the count
 * in the message. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossHits(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* targets, const long long* targetOffsets, int numTargets,
    EdlibAlignConfig config, int device);

/* The hits of the last Run of such a batch: every cell whose editDistance is not -1, i.e. exactly the cells of the
 * dense batch's matrix that are not -1, grouped by target (CSR) and by ascending query index inside a target.
 * Pointers into pinned memory the batch owns, valid until the next Run / Destroy. */
typedef struct {
    int numQueries, numTargets;
    long long numHits;
    const long long* targetOffsets;   /* [numTargets + 1]: hits of target t are [targetOffsets[t], targetOffsets[t+1]) */
    const int* query;                 /* [numHits] */
    const int* editDistance;          /* [numHits] */
    const int* numLocations;          /* [numHits] */
    const int* endLocation;           /* [numHits] endLocations[0], else -1 */
} EdlibAmdCrossHits;
EDLIB_API int edlibAmdBatchCrossHits(EdlibAmdBatch* batch, EdlibAmdCrossHits* out);

/* A cross batch whose results are, per (query, target) cell, EVERY occurrence of the query within k along the target (an
 * occurrence batch) -- adapter and primer trimming, a barcode at both ends of a read, concatemer splitting, repeats of a
 * motif per read: the questions of a hit-list read batch asked of many targets at once, which a hit-list cross
 * batch (one best cell per pair) and any number of edlibAlign() calls with a k do not answer.
 * For query q of length m and target t of length n, D[j] (j = 0 .. n-1) is the HW bottom-row score -- the least edit
 * distance between q and any substring of t that ends at column j (the empty one counts: D[j] <= m; there is no column
 * -1 here).  An OCCURRENCE is a maximal run [firstEnd, lastEnd] of consecutive columns with D[j] <= k; its editDistance
 * is the least D of the run, endLocation the lowest column of the run holding it, numLocations the number of columns of
 * the run holding it; all columns are relative to the target's own first base.  The least editDistance over a cell's
 * occurrences equals edlibAlign(q, t, HW, k).editDistance, a cell without one is -1 there (n > 0), and every non-negative
 * end location of that call lies in an occurrence of that distance.  k >= m gives one occurrence [0, n-1] per non-empty
 * target; an empty query occurs once in every non-empty target: [0, n-1], distance 0, endLocation 0, numLocations n; an
 * empty target holds no occurrence.
 * Accepted: config.mode == EDLIB_MODE_HW, config.task == EDLIB_TASK_DISTANCE, config.k >= 0, every query at most 256
 * bases, every target with at most 16 distinct symbols of its own; additionalEqualities allowed; numQueries == 0 and
 * numTargets == 0 are valid.  Anything else (NW / SHW, EDLIB_TASK_LOC / EDLIB_TASK_PATH, k < 0, a longer query, a target
 * with more symbols, a bad shape or bad offsets) returns NULL with the limit named in edlibAmdLastError(); all of these
 * are checked before the device is looked for.
 * Targets up to 65,536 bases run on the cross kernel when the union alphabet of all targets has at most 16 symbols;
 * every other target runs all queries through one internal hit-list shared-target session, and its occurrences take
 * their place in the list.
 * Run, Stats and Destroy work as for a cross batch: Stats.path has bit 3 set when the kernel ran and bit 0 as well when
 * an internal session ran; Stats.cells and Stats.word_steps are those of an HW edlibAmdBatchCreateCrossHits batch over
 * the same inputs (an internal session adds the word-steps it executed).  edlibAmdBatchCrossOccurrences has the results;
 * CrossView, CrossHits, CrossStrands and the views of every other kind fail.
 * The device list starts at max(2^20, numQueries + numTargets) runs; a Run that counts more grows it to its count and
 * scans once more (later Runs of the batch fit); a list that does not fit in device memory fails the Run with the count
 * in the message, and so does one of more than 2^32 - 1 runs.
 * Out of scope: both strands (pass the reverse complements as queries of their own -- there is one level, so nothing to
 * prune); start locations and paths (align the chosen windows with a pair or window batch); best-per-target and
 * best-per-query reductions (a hit-list cross batch has those). */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossOccurrences(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* targets, const long long* targetOffsets, int numTargets,
    EdlibAlignConfig config, int device);

/* The occurrences of the last Run of such a batch (it fails on every other kind, and before the first Run), made on the
 * device and copied as one block (the offsets, then six int planes): pointers into pinned memory the batch owns, valid
 * until the next Run / Destroy.  Occurrences are grouped by target in the caller's order (CSR), inside a target by
 * ascending query index, inside a cell by ascending firstEnd (lastEnd + 1 < the next firstEnd: runs are maximal). */
typedef struct {
    int numQueries, numTargets; long long numHits;
    const long long* targetOffsets;   /* [numTargets + 1]: occurrences in target t are [targetOffsets[t], targetOffsets[t+1]) */
    const int* query;                 /* [numHits] */
    const int* firstEnd;  const int* lastEnd;                                   /* [numHits] each */
    const int* editDistance;  const int* endLocation;  const int* numLocations; /* [numHits] each */
} EdlibAmdCrossOccurrences;
EDLIB_API int edlibAmdBatchCrossOccurrences(EdlibAmdBatch* batch, EdlibAmdCrossOccurrences* out);

/* Replace the target set of a resident cross batch.  The queries, their Peq slots, the config, the device, the stream,
 * the hit-list capacity a previous Run grew to and the pinned view blocks stay; everything derived from the targets is
 * made again.  Afterwards the batch is as if it had been created over (its queries, these targets): Run, then the views.
 * Returns 0, or non-zero with edlibAmdLastError().
 * Valid on the batches of edlibAmdBatchCreateCross, ...CrossHits, ...CrossOccurrences, ...CrossBothStrands and
 * ...CrossHitsBothStrands; refused on self batches, window batches and every other kind.
 * A streamed set lies inside the cross kernel's envelope: every target at most 65,536 bases, at most 16 distinct symbols
 * over all targets, and no query of the batch above 256 bases.  Outside it the call is refused with the limit named
 * ("... create a new batch"): a streamed set builds no internal sessions, and those a Create built are dropped by the
 * first successful call.  targetOffsets[0] need not be 0; the caller's memory may be reused when the call returns;
 * numTargets == 0 is valid (Run succeeds, the views are empty).
 * A refusal (a NULL or wrong-kind batch, numTargets < 0, a NULL pointer with numTargets > 0, offsets that decrease, the
 * three limits above) leaves the batch as it was: the previous targets, the views of the last Run, the results of the
 * next.  A device error (out of memory) may leave the batch without targets: Run and the views then fail with a message
 * that says so until a SetTargets succeeds.  After success the views fail ("Run it first") until the next Run, and
 * Stats.cells describes the new set.
 * The targets are prepared on the device (alphabet census, stable sort by length, packing); the host's share is linear in
 * numTargets. */
EDLIB_API int edlibAmdBatchCrossSetTargets(EdlibAmdBatch* batch, const char* targets,
                                           const long long* targetOffsets, int numTargets);

/* Cross batches on both strands: as edlibAmdBatchCreateCross / edlibAmdBatchCreateCrossHits (the same arguments, routing
 * and refusals, checked before the device is looked for: task other than EDLIB_TASK_DISTANCE, unknown mode, k < 0 for the
 * hit-list form), but cell (q, t) is the better of edlibAlign(query q, target t, config) and
 * edlibAlign(revcomp(query q), target t, config), chosen by the table above edlibAmdBatchCreateSharedBothStrands: the
 * forward strand wins a tie, the winner's editDistance, numLocations and first end location are reported, and a cell
 * that is -1 on both strands is the forward record with -1.  revcomp is edlibAmdReverseComplement, made on the device from
 * the uploaded pool.  (A barcode or adapter sits on either strand of a read: with the reverse complements passed as
 * queries of their own, a query's other strand competes with it as the runner-up of every best hit.)
 * edlibAmdBatchCrossView (MATRIX, BEST) and edlibAmdBatchCrossHits work as on the plain batches and describe the COMBINED
 * cells: numQueries wide, a hit is a combined cell that is not -1 (one per (q, t)), best and second best run over the
 * combined cells with the same tie and index rules, so a query's other strand is never its own runner-up.
 * edlibAmdBatchCrossStrands says which strand every cell reports; StrandView and the views of the other kinds fail.
 * Stats.cells and Stats.word_steps count both strands; Stats.path bit 3 as for a plain cross batch.  On the cross kernel
 * a query and its reverse complement are neighbouring lanes of a wave and the choice is one lane exchange per cell. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossBothStrands(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* targets, const long long* targetOffsets, int numTargets,
    EdlibAlignConfig config, int device);
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateCrossHitsBothStrands(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* targets, const long long* targetOffsets, int numTargets,
    EdlibAlignConfig config, int device);

/* The strands of the last Run of such a batch (it fails on every other kind, and before the first Run): pointers into
 * pinned memory the batch owns, valid until the next Run / Destroy.  A strand byte has bit 0 set when the cell reports
 * the reverse complement and bit 1 set when the other strand reaches the same distance (then bit 0 is clear: ties go
 * forward); it is 0 for a -1 cell and for a best that is -1.  `what`: EDLIB_AMD_CROSS_MATRIX asks for the byte of every
 * cell -- cellStrand of a dense batch, hitStrand of a hit-list batch --, EDLIB_AMD_CROSS_BEST for the bytes of the best
 * hits of edlibAmdBatchCrossView; the parts not asked for, and the part of the other form, are NULL. */
typedef struct {
    int numQueries, numTargets; long long numHits;
    const unsigned char* cellStrand;        /* [numTargets * numQueries]  dense batches, asked with EDLIB_AMD_CROSS_MATRIX */
    const unsigned char* hitStrand;         /* [numHits]                  hit-list batches, in the order of EdlibAmdCrossHits */
    const unsigned char* bestQueryStrand;   /* [numTargets]               asked with EDLIB_AMD_CROSS_BEST */
    const unsigned char* bestTargetStrand;  /* [numQueries] */
} EdlibAmdCrossStrands;
EDLIB_API int edlibAmdBatchCrossStrands(EdlibAmdBatch* batch, int what, EdlibAmdCrossStrands* out);

/* One set of numSequences sequences against itself (a self batch): replaces
 *   for i: for j > i: d(i, j) = edlibAlign(seq i, .., seq j, .., config).editDistance
 * (UMI / barcode de-duplication, barcode-set design checks, amplicon and sequence clustering, distance matrices for trees)
 * with every unordered pair computed once -- NW distance is symmetric, and so are additionalEqualities -- and the set
 * uploaded, packed and profiled once; a cross batch given the same pool twice scans every pair twice.  d(i, j) is what a
 * cross batch reports for query i against target j: -1 above k or where the lengths differ by more than k, and for an
 * empty sequence the other's length whatever k.  numLocations and endLocation are not reported (NW: 1 and length - 1).
 * Accepted: config.mode == EDLIB_MODE_NW, config.task == EDLIB_TASK_DISTANCE, any k (CreateSelfHits: k >= 0),
 * additionalEqualities; anything else returns NULL with the reason in edlibAmdLastError(), as do numSequences < 0 and
 * offsets that descend -- all checked before the device is.  numSequences 0 and 1 are valid batches without a pair.
 * edlibAmdBatchCreateSelf keeps the distances as a condensed vector (n (n - 1) / 2 ints on the device);
 * edlibAmdBatchCreateSelfHits keeps only the pairs within k, as a list that starts at max(2^20, 2 n) hits and grows as a
 * hit-list cross batch's does.  Pairs of sequences up to 256 bases over at most 16 symbols run on the self instantiation
 * of the cross kernel; pairs with a longer sequence, and every pair of a set with more symbols, run through one internal
 * pair batch over the i < j pairs inside the length window (at most 2^31 - 1 of them).
 * Run, Stats and Destroy work as for a cross batch (Stats.path bit 3: the kernel, bit 1: the pair batch; Stats.cells the
 * sum of length i * length j over i < j; Stats.word_steps the sum of ceil(min / 32) * max of the two lengths over the
 * pairs the kernel scans); every other view (Results.., CigarView, StrandView, CrossView, CrossHits, CrossStrands,
 * SharedHits, WindowView) fails and names the self views. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelf(
    const char* seqs, const long long* offsets, int numSequences, EdlibAlignConfig config, int device);
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfHits(
    const char* seqs, const long long* offsets, int numSequences, EdlibAlignConfig config, int device);

/* Results of the last Run of a self batch (it fails on every other kind, and before the first Run), as pointers into
 * pinned host memory the batch owns (valid until the next Run / Destroy).  Only the parts asked for in `what`
 * (EDLIB_AMD_SELF_DISTANCES | EDLIB_AMD_SELF_NEAREST) cross the link.
 * editDistance is in condensed order (scipy's pdist / squareform): pair (i, j), i < j, is at
 * numSequences * i - i * (i + 1) / 2 + (j - i - 1), computed in 64 bits; it is NULL when not asked for and in a hit-list
 * batch.  Nearest, of both kinds of batch: over all OTHER sequences, on either side of the triangle, the smallest
 * (distance << 32) | partner wins, so ties go to the lowest index; secondDistance is the smallest distance over the
 * remaining partners (equal to the best on a tie); all three are -1 where no other sequence is within k. */
typedef struct {
    int numSequences;
    long long numPairs;               /* numSequences * (numSequences - 1) / 2                       */
    const int* editDistance;          /* [numPairs] condensed, -1: above k                           */
    const int* nearest;               /* [numSequences]                                              */
    const int* nearestDistance;       /* [numSequences]                                              */
    const int* secondDistance;        /* [numSequences]                                              */
} EdlibAmdSelfView;
#define EDLIB_AMD_SELF_DISTANCES 1
#define EDLIB_AMD_SELF_NEAREST   2
EDLIB_API int edlibAmdBatchSelfView(EdlibAmdBatch* batch, int what, EdlibAmdSelfView* out);

/* The hits of the last Run of a hit-list self batch: every pair i < j whose distance is not -1, exactly once, grouped by
 * i (CSR) with the partners j > i ascending inside a row; no (i, i) entry.  Pinned memory the batch owns, valid until the
 * next Run / Destroy. */
typedef struct {
    int numSequences;
    long long numHits;
    const long long* rowOffsets;      /* [numSequences + 1]: partners of i are [rowOffsets[i], rowOffsets[i+1]) */
    const int* partner;               /* [numHits] j > i */
    const int* editDistance;          /* [numHits] */
} EdlibAmdSelfHits;
EDLIB_API int edlibAmdBatchSelfHits(EdlibAmdBatch* batch, EdlibAmdSelfHits* out);

/* A hit-list self batch over a partitioned set (UMIs per cell and gene, clonotypes per V/J gene or sample, duplicates per
 * locus): groups[i] is any int label of sequence i, negative values included; sequences with equal labels form a group,
 * which need not be contiguous in the input.  Pair (i, j), i < j, exists only where groups[i] == groups[j], and every view
 * -- edlibAmdBatchSelfHits, edlibAmdBatchSelfView with EDLIB_AMD_SELF_NEAREST, edlibAmdBatchSelfComponents,
 * edlibAmdBatchSelfNeighbors, a pair batch filled by edlibAmdBatchPairsSetCells -- reports exactly what
 * edlibAmdBatchCreateSelfHits over each group alone would, with that group's indices mapped back to the whole set:
 * partners ascend inside a row, the key rule of nearest and neighbours is unchanged, and a pair with an empty sequence is
 * the other's length whatever k, inside a group only.  One Create, one upload and one launch sequence whatever the number
 * of groups; pairs across groups are neither scanned nor listed.
 * Accepted: what edlibAmdBatchCreateSelfHits accepts (NW, DISTANCE, k >= 0, additionalEqualities); groups == NULL is
 * refused and names edlibAmdBatchCreateSelfHits.  There is no dense grouped form (a condensed vector has no meaning across
 * groups: EdlibAmdSelfView.editDistance stays NULL, numPairs counts the pairs inside groups) and no both-strand one.
 * Routing is a self batch's, inside groups: sequences up to 256 bases over at most 16 symbols in the whole set on the
 * grouped instantiation of the self kernel (Stats.path bit 3), same-group pairs with a longer sequence and every
 * same-group pair of a set with more symbols through one internal pair batch (bit 1; at most 2^31 - 1 pairs).
 * Stats.cells is the sum over groups of the sum of length i * length j over i < j; Stats.word_steps the sum of
 * ceil(min / 32) * max over the same-group pairs the kernel scans (both with bases, both <= 256, lengths within k). */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfHitsGrouped(
    const char* seqs, const long long* offsets, int numSequences, const int* groups, EdlibAlignConfig config, int device);

/* Self batches on both strands (sequences of unknown orientation: amplicons, UMIs, barcodes, k-mer sets): the same
 * arguments, routing and refusals as the two Creates above -- checked before the device is looked for, with the same
 * messages, and numSequences above 0x3fffffff is refused too -- but pair (i, j), i < j, is the better of
 *   fwd = edlibAlign(seq i, seq j, config).editDistance  and  rev = edlibAlign(revcomp(seq i), seq j, config).editDistance
 * by the table above edlibAmdBatchCreateSharedBothStrands: the forward orientation wins a tie, and the pair is -1 where
 * neither is within k.  revcomp is edlibAmdReverseComplement of the LOWER-INDEXED sequence.  With c the complement of a
 * byte and Eq the match relation (identity and additionalEqualities, both directions), that equals the reverse complement
 * of the other sequence against this one exactly when Eq(c(x), y) <=> Eq(x, c(y)) for all bytes x, y present in the set:
 * true for ACGT, ACGTN, mixed case and IUPAC codes whose equalities are closed under complement; false where U or u is
 * present (c(U) = A, c(A) = T) and for an equality such as (R, A) without (Y, T).  Create evaluates the condition over
 * the bytes present.  Where it holds, pairs inside the kernel's envelope run on the self kernel with the two
 * orientations of a pair in neighbouring lanes (Stats.path bit 3); where it fails, EVERY pair runs through the internal
 * pair batch in index order (Stats.path bit 3 stays clear), so the answers equal the definition either way.  A pair with
 * an empty sequence is the other's length on both orientations.
 * edlibAmdBatchSelfView and edlibAmdBatchSelfHits work unchanged and describe the COMBINED distances; nearest,
 * nearestDistance and secondDistance run over them with the same key rule.  Stats.cells and Stats.word_steps count both
 * orientations (twice a one-strand self batch's). */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfBothStrands(
    const char* seqs, const long long* offsets, int numSequences, EdlibAlignConfig config, int device);
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSelfHitsBothStrands(
    const char* seqs, const long long* offsets, int numSequences, EdlibAlignConfig config, int device);

/* The strand bytes of the last Run of such a batch (it fails on a one-strand self batch, on every other kind, on NULL
 * and before the first Run, with the reason in edlibAmdLastError()): pointers into pinned memory the batch owns, valid
 * until the next Run / Destroy.  A strand byte has bit 0 set when the reverse orientation is reported and bit 1 set when
 * the other orientation reaches the same distance (then bit 0 is clear: ties go forward); it is 0 where the distance is
 * -1.  `what`: EDLIB_AMD_SELF_DISTANCES asks for the byte of every pair -- pairStrand of a dense batch, hitStrand of a
 * hit-list batch --, EDLIB_AMD_SELF_NEAREST for nearestStrand, the byte of the pair (x, nearest[x]), 0 where nearest is
 * -1; the parts not asked for, and the part of the other form, are NULL. */
typedef struct {
    int numSequences;
    long long numPairs;
    long long numHits;
    const unsigned char* pairStrand;    /* [numPairs]     dense batches, condensed order, asked with EDLIB_AMD_SELF_DISTANCES */
    const unsigned char* hitStrand;     /* [numHits]      hit-list batches, in the order of edlibAmdBatchSelfHits           */
    const unsigned char* nearestStrand; /* [numSequences] asked with EDLIB_AMD_SELF_NEAREST                                 */
} EdlibAmdSelfStrands;
EDLIB_API int edlibAmdBatchSelfStrands(EdlibAmdBatch* batch, int what, EdlibAmdSelfStrands* out);

/* The connected components of the last Run of a self batch (single linkage: UMI / barcode collapsing, amplicon and OTU
 * clustering, clonotype grouping, duplicate removal), labelled on the device from the pairs where the Run left them --
 * the finished hit list or the condensed vector -- so that numSequences ints cross the link instead of the pairs.
 * With L = maxDistance if it is >= 0, else the batch's k (and if that is < 0 too, every reported pair counts), the graph
 * has the sequences as vertices and an edge {i, j} for every pair whose distance d, as edlibAmdBatchSelfView /
 * edlibAmdBatchSelfHits report it (both strands: the combined distance), satisfies 0 <= d, and d <= L when L >= 0.  An
 * empty sequence is reported at the other's length whatever k, so under d <= L it joins only sequences of length <= L:
 * its true edit distance.  One Run at k serves every level up to k: call it any number of times per Run.
 * label[i] is the SMALLEST index in i's component -- canonical, independent of the order in which the device meets the
 * edges, equal bit for bit to a union-find on the host; numComponents is the number of i with label[i] == i;
 * componentSize[i] the number of sequences in i's component.  With EDLIB_AMD_COMPONENT_MEMBERS the components are listed
 * in ascending order of their labels, the members ascending inside each: component c is
 * members[componentOffsets[c] .. componentOffsets[c + 1]), and label[members[componentOffsets[c]]] is the c-th smallest
 * label.  The label parts are always filled.
 * All four kinds of self batch are accepted, after a successful Run; numSequences 0 and 1 are valid (no component, one
 * of size 1).  The pointers are pinned memory the batch owns, valid until the next edlibAmdBatchSelfComponents, Run or
 * Destroy.  Refused with the reason in edlibAmdLastError(), the batch and its other views (and pointers a caller holds
 * from them) left as they were: `what` 0 or with unknown bits, NULL batch or out, any other kind of batch, a batch that
 * has not run, and maxDistance > k on a batch with k >= 0 (it kept no pairs beyond k).  Stats are untouched. */
typedef struct {
    int numSequences;
    int numComponents;
    const int* label;             /* [numSequences]      the LOWEST index in i's component            */
    const int* componentSize;     /* [numSequences]      number of sequences in i's component         */
    const int* componentOffsets;  /* [numComponents + 1] asked with EDLIB_AMD_COMPONENT_MEMBERS, else NULL */
    const int* members;           /* [numSequences]      likewise: sequences grouped by component     */
} EdlibAmdSelfComponents;
#define EDLIB_AMD_COMPONENT_LABELS  1
#define EDLIB_AMD_COMPONENT_MEMBERS 2
EDLIB_API int edlibAmdBatchSelfComponents(EdlibAmdBatch* batch, int maxDistance, int what, EdlibAmdSelfComponents* out);

/* The K nearest neighbours per row of the last Run, selected on the device from the results where the Run left them --
 * the condensed vector, the matrix or the finished hit list -- so that numRows x K entries cross the link instead of the
 * pairs or cells (kNN graphs for clustering, the few candidate barcodes of an ambiguous read, the K closest references).
 * edlibAmdBatchSelfNeighbors: a row is a sequence i of a self batch (all four kinds), its candidates the OTHER sequences
 * j != i on both sides of the triangle, at the distance edlibAmdBatchSelfView / edlibAmdBatchSelfHits report for the pair.
 * edlibAmdBatchCrossNeighbors: a row is a target t of a cross batch (dense or hit list, one strand or both), its
 * candidates the queries, at the distance of cell (t, q).  Neighbours of the queries are not offered.
 * A candidate takes part where its distance d satisfies 0 <= d and, with maxDistance >= 0, d <= maxDistance; with
 * maxDistance < 0 every distance the batch reports counts (also the pairs of an empty sequence, which a self batch
 * reports at the other's length whatever k).  A row lists its count[row] <= K
 * nearest candidates in ascending order of the key (distance << 32) | index: the smaller distance first, ties to the
 * lower index -- the rule of the nearest / best views, so with maxDistance = -1 neighbor[row][0], distance[row][0] and
 * distance[row][1] equal nearest, nearestDistance and secondDistance (bestQuery, bestQueryDistance, secondQueryDistance).
 * Entries past count[row] are -1 / -1 / strand 0.  strand[row][r] (both-strand batches) is the strand byte of that pair
 * or cell as edlibAmdBatchSelfStrands / edlibAmdBatchCrossStrands report it.
 * K is 1..64.  Valid after a successful Run, any number of times per Run; numRows 0, a single sequence and numQueries 0
 * are valid (no rows / count 0).  The pointers are pinned memory the batch owns, valid until the next Neighbors call,
 * Run, edlibAmdBatchCrossSetTargets or Destroy.  Refused with the reason in edlibAmdLastError(), the batch and its other
 * views (and pointers a caller holds from them) left as they were: K out of range, NULL batch or out, the other kind of
 * batch, an occurrence batch (its entries are runs, not cells), a batch that has not run (a cross batch that took new
 * targets since its last Run has not), and maxDistance > k on a batch with k >= 0.  Stats are untouched. */
typedef struct {
    int numRows;                 /* sequences (self) or targets (cross)                         */
    int K;
    const int* count;            /* [numRows]     neighbours reported for the row, 0..K         */
    const int* neighbor;         /* [numRows][K]  ascending by (distance, index); -1 past count */
    const int* distance;         /* [numRows][K]  -1 past count                                 */
    const unsigned char* strand; /* [numRows][K]  both-strand batches only, else NULL; 0 past count */
} EdlibAmdNeighbors;
EDLIB_API int edlibAmdBatchSelfNeighbors(EdlibAmdBatch* batch, int K, int maxDistance, EdlibAmdNeighbors* out);
EDLIB_API int edlibAmdBatchCrossNeighbors(EdlibAmdBatch* batch, int K, int maxDistance, EdlibAmdNeighbors* out);

/* A shared-target batch whose results are, per read, EVERY occurrence within k along the target -- the search question of
 * adapter / primer trimming, concatemer splitting, repeat finding and multi-mapping reads, which no choice of k makes
 * edlibAlign() answer (it keeps the columns of the single best score only).
 * With m = the read's length, T = targetLength and D[j] (j = 0 .. T-1) the HW bottom-row score -- the least edit distance
 * between the read and any substring of the target that ends at column j (the empty one counts: D[j] <= m; there is no
 * column -1 here) -- a HIT is a maximal run [firstEnd, lastEnd] of consecutive columns with D[j] <= k.  Its editDistance is
 * the least D of the run, endLocation the lowest column of the run holding it, numLocations the number of columns of the
 * run holding it.  The least editDistance over a read's hits equals edlibAlign(read, target, HW, k).editDistance, no hit
 * means -1 there, and every non-negative end location of that call lies in a hit of that distance.
 * Accepted: config.mode == EDLIB_MODE_HW, config.task == EDLIB_TASK_DISTANCE, config.k >= 0, every read at most 256 bases,
 * at most 16 distinct target symbols; additionalEqualities allowed.  Anything else (SHW / NW, start locations and paths,
 * longer reads, more symbols) returns NULL with the limit named in edlibAmdLastError().  For both strands pass the reverse
 * complements as reads of their own (this kind has no both-strand form); for start locations or paths align the chosen windows with a pair batch.
 * An empty read hits once: [0, T-1], distance 0, endLocation 0, numLocations T; an empty target gives no hit.
 * Run, Stats (path bit 0) and Destroy work as for a shared batch; Results, ResultsFlat, ResultsView, CigarView, StrandView,
 * CrossView and CrossHits fail.  The device list starts at max(2^20, numQueries) runs; a Run that counts more grows it to
 * its count and scans once more (later Runs of the batch fit); a list that does not fit in device memory fails the Run with
 * the count in the message. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateSharedHits(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* target, int targetLength, EdlibAlignConfig config, int device);

/* The hits of the last Run of such a batch (it fails on every other kind), made on the device and copied as one block:
 * pointers into pinned memory the batch owns, valid until the next Run / Destroy.  Hits are grouped by read in the caller's
 * order (CSR) and ascend by firstEnd inside a read. */
typedef struct {
    int numUnits; long long numHits;
    const long long* unitOffsets;   /* [numUnits + 1]: hits of read i are [unitOffsets[i], unitOffsets[i+1]) */
    const int* firstEnd;            /* [numHits] */
    const int* lastEnd;             /* [numHits] */
    const int* editDistance;        /* [numHits] */
    const int* endLocation;         /* [numHits] */
    const int* numLocations;        /* [numHits] */
} EdlibAmdReadHits;
EDLIB_API int edlibAmdBatchSharedHits(EdlibAmdBatch* batch, EdlibAmdReadHits* out);

/* numUnits units over ONE resident target (a window batch): unit u is query unitQuery[u] against the window
 * target[unitStart[u] .. unitStart[u] + unitLength[u]).  Replaces
 *   for u: r[u] = edlibAlign(query(unitQuery[u]), .., target + unitStart[u], unitLength[u], config)
 * (the verification step of a seed-and-extend mapper: a read against a few candidate loci of one reference) without
 * replicating a byte of the target or of a query: the target is uploaded and packed once, every query once, and the
 * units are three ints each.  config.task must be EDLIB_TASK_DISTANCE (for locations or paths align the chosen units
 * with a pair batch, as for cross batches); NW, SHW and HW, any k, additionalEqualities.
 * Create returns NULL, with the limit named in edlibAmdLastError(), for another task, numUnits < 0, and for a unit with
 * unitQuery outside [0, numQueries), unitStart < 0, unitLength < 0 or unitStart + unitLength > targetLength (the message
 * names the first such unit); these are checked before the device is.  numUnits == 0 is a valid batch.
 * Units of queries up to 256 bases against windows up to 65,536 columns of a target with at most 16 distinct symbols
 * run on the window kernel.  Every other unit runs through one internal pair batch over slices copied at Create: that
 * route DOES replicate bytes -- right for a handful of long reads, and for a protein target the cost of a pair batch.
 * Run, Stats and Destroy work as for the other batches (Stats.path bit 4: the window kernel, bit 1: the internal pair
 * batch ran; Stats.cells the sum of queryLength * unitLength); Results, ResultsFlat, ResultsView, CigarView, StrandView,
 * CrossView, CrossHits and SharedHits fail. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateWindows(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* target, int targetLength,
    const int* unitQuery, const int* unitStart, const int* unitLength, int numUnits,
    EdlibAlignConfig config, int device);

/* As edlibAmdBatchCreateWindows with a strand per unit (a mapper's candidates are (read, locus, strand)): unit u is
 * revcomp(query unitQuery[u]) against its window where unitStrand[u] == 1 and the query itself where it is 0; revcomp is
 * edlibAmdReverseComplement, made on the device from the uploaded pool.  A NULL unitStrand is all forward and equals
 * edlibAmdBatchCreateWindows.  Any other value is refused, naming the first such unit, with the other unit checks (before
 * the device).  edlibAmdBatchWindowView is unchanged: units as defined here, and the best per query runs over ALL units
 * that name the query, whatever their strand, by the same key rule -- the winner's strand is unitStrand[bestUnit].
 * Stats as for a plain window batch. */
EDLIB_API EdlibAmdBatch* edlibAmdBatchCreateWindowsStranded(
    const char* queries, const long long* queryOffsets, int numQueries,
    const char* target, int targetLength,
    const int* unitQuery, const int* unitStart, const int* unitLength, const unsigned char* unitStrand, int numUnits,
    EdlibAlignConfig config, int device);

/* Results of the last Run of a window batch (it fails on every other kind, and before the first Run), as pointers into
 * pinned host memory the batch owns (valid until the next Run / Destroy).  Only the parts asked for in `what`
 * (EDLIB_AMD_WINDOW_UNITS | EDLIB_AMD_WINDOW_BEST) cross the link; the others are NULL.
 * Unit u equals its edlibAlign() call above in editDistance (-1: above k), numLocations and the first end location (-1
 * when there is none) -- the contract of a cross batch's cell.  End locations are WINDOW-relative, as that call returns
 * them: add unitStart[u] to a non-negative one for the target coordinate.
 * Best per query, over the units that name it: the smallest (distance << 32) | unit index wins, so ties go to the lowest
 * unit index; secondDistance is the smallest distance over the query's other units (equal to the best on a tie); a query
 * with no unit within k, or no unit at all, has -1 in all three. */
typedef struct {
    int numUnits, numQueries;
    const int* editDistance;     /* [numUnits] -1: above k                                   */
    const int* numLocations;     /* [numUnits]                                               */
    const int* endLocation;      /* [numUnits] endLocations[0] of that call, WINDOW-relative */
    const int* bestUnit;         /* [numQueries] */
    const int* bestDistance;     /* [numQueries] */
    const int* secondDistance;   /* [numQueries] */
} EdlibAmdWindowView;
#define EDLIB_AMD_WINDOW_UNITS 1
#define EDLIB_AMD_WINDOW_BEST  2
EDLIB_API int edlibAmdBatchWindowView(EdlibAmdBatch* batch, int what, EdlibAmdWindowView* out);

/* Replace the queries and the units of a resident window batch (a mapper's next chunk of reads and candidates over the
 * same reference).  The target, its 4-bit pack, its tables, the config, the device, the stream, the pinned view blocks
 * and every device buffer that is large enough stay; the query pool, the unit list and everything derived from them are
 * made again.  Afterwards the batch is as if it had been created over (its target, its config, these queries, these
 * units): Run, then edlibAmdBatchWindowView.  Returns 0, or non-zero with edlibAmdLastError().
 * Valid on the batches of edlibAmdBatchCreateWindows and ...WindowsStranded, whichever of the two created it: a NULL
 * unitStrand is all forward, a stranded set may follow a plain one and the other way round.  Refused, with this function
 * and the kind named, on cross, self, read and pair batches.
 * A streamed set lies inside the window kernel's envelope: the batch's target has at most 16 distinct symbols (decided
 * at Create: a batch over a wider target refuses every call), every query is at most 256 bases -- named by a unit or not
 * -- and every window at most 65,536 columns.  Outside it the call is refused with the first offending query or unit, its
 * size and the limit named ("... create a new batch"): a streamed set builds no internal pair batch, and the one a
 * Create built is dropped by the first successful call.  The unit checks are those of Create, with its messages:
 * unitQuery outside [0, numQueries), a negative unitStart or unitLength, unitStart + unitLength > targetLength,
 * unitStrand > 1.  Also refused: numUnits < 0, numQueries < 0, a NULL pointer with a positive count, query offsets that
 * decrease.  queryOffsets[0] need not be 0; the caller's memory may be reused when the call returns; numUnits == 0 and
 * numQueries == 0 are valid (Run succeeds, the views are empty).
 * Every refusal is decided before the batch changes and leaves it as it was: the previous queries and units, the views
 * of the last Run (pointers the caller still holds included), the results of the next.  Behind that point only a device
 * error (out of memory) can fail the call; it may leave the batch without units: Run and the views then fail with a
 * message that says so until a SetUnits succeeds.  After success the views fail ("Run it first") until the next Run, and
 * Stats.cells describes the new set.
 * The set is prepared on the device (word groups, stable sort by window length, a Peq slot per query and strand a unit
 * names); the host's share is one pass over the offsets and one over the units, and it reads no byte of a query. */
EDLIB_API int edlibAmdBatchWindowsSetUnits(EdlibAmdBatch* batch,
    const char* queries, const long long* queryOffsets, int numQueries,
    const int* unitQuery, const int* unitStart, const int* unitLength,
    const unsigned char* unitStrand /* NULL: all forward */, int numUnits);

/* Replace the pairs of a resident pair batch (a mapper's next chunk of winners, whose start locations or paths are
 * wanted).  The config with its equalities, the device, the stream, the pinned view blocks and every device buffer that
 * is large enough stay; the pools, the offsets and everything derived from the pairs are made again.  Afterwards the batch
 * is as if it had been created over (its config, its device, these pairs): Run, then edlibAmdBatchResults, ...ResultsFlat,
 * ...ResultsView, ...CigarView, ...Stats.  Returns 0, or non-zero with edlibAmdLastError().
 * Valid on the batches of edlibAmdBatchCreatePairs, whatever they were created over: zero pairs, a handful, a set with a
 * long pair or an empty sequence (the state of their general path is dropped by the first successful call).  Refused, with
 * this function and the kind named, on shared-target, both-strand and hit-list read batches and on cross, self,
 * occurrence and window batches.
 * A streamed set is a flat set: every query has 1 to 1,024 bases and every target 1 to 65,536; under
 * EDLIB_TASK_PATH also SHW / HW queries have at most 256 bases, no pair reaches the linear-space regime (the reference's
 * 1 MiB rule) and the column stores and op slots of the set stay below 32 GB / 8 GB.  The count is free: numPairs from 0
 * up, the last chunk of a stream is usually short.  Outside the envelope the call is refused with the first offending
 * pair, its size and the limit named ("... create a new batch").  Also refused: numPairs < 0, a NULL pointer with a
 * positive count, offsets that decrease.  The offsets need not start at 0; the caller's memory may be reused when the call
 * returns; numPairs == 0 is valid (Run succeeds, the views are empty).
 * Every refusal is decided from the offsets and the config alone, before the batch changes, and leaves it as it was: the
 * previous pairs, the views of the last Run (pointers the caller still holds included), the results of the next.  Behind
 * that point only a device error (out of memory) can fail the call; it may leave the batch without pairs: Run and the
 * views then fail with a message that says so until a SetPairs succeeds.  After success the views fail ("Run it first")
 * until the next Run, and Stats.cells describes the new set.
 * The set is prepared on the device (a census of the target bytes for the alphabet, exclusive scans for the Peq offsets,
 * op slots and store bases, the descriptors by a kernel); the host's share is one pass over the two offset arrays, and it
 * reads no byte of a sequence. */
EDLIB_API int edlibAmdBatchPairsSetPairs(EdlibAmdBatch* batch,
    const char* queries, const long long* queryOffsets,
    const char* targets, const long long* targetOffsets, int numPairs);

/* Replace the pairs of a resident pair batch by pairs named over a window batch and gathered on the device (a mapper's
 * winners of edlibAmdBatchWindowView, without the slices leaving the device): the query of pair i is query pairQuery[i]
 * of `windows` -- its edlibAmdReverseComplement where pairStrand[i] == 1 -- and its target is
 * target[pairStart[i] .. pairStart[i] + pairLength[i]) of the target of `windows`.  Afterwards `pairs` is exactly the
 * batch edlibAmdBatchPairsSetPairs would have made over these pairs materialised: everything that call keeps and resets
 * this one keeps and resets, and Run, Results, ResultsFlat, ResultsView, CigarView and Stats follow as there.  Returns 0,
 * or non-zero with edlibAmdLastError().  The tuples are the caller's own, not unit indices of `windows`: a padded window
 * around a verified one, a second-best unit, any strand.
 * The bytes are copied: when the call returns `pairs` depends on nothing in `windows`, which may be given new units, run
 * or destroyed.  `windows` is not changed in any way a caller can observe: the views of its last Run, its next Run and
 * its Stats stay as they were.
 * `pairs` is a batch of edlibAmdBatchCreatePairs in any state SetPairs accepts.  `windows` is a window batch whose current
 * set was prepared on the device -- by a Create whose units all lie inside the window kernel's envelope, or by any
 * successful edlibAmdBatchWindowsSetUnits; then its query pool (both strands where a unit named one) and the 4-bit pack
 * of its target are resident.  Any number of Runs may have happened, none included.
 * Refused, with this function and the reason named: a NULL handle; another kind of batch on either side (the kind is
 * named as SetPairs names it); batches on different devices; a `windows` over a target with more than 16 distinct symbols;
 * a `windows` whose Create took the host route (a unit outside the envelope: nothing is resident to gather from); a
 * `windows` left without units by a SetUnits that failed on the device; numPairs < 0; a NULL pairQuery, pairStart or
 * pairLength with a positive count (a NULL pairStrand is all forward).  Per pair, the first offender named with its
 * values: pairQuery outside [0, numQueries) of `windows`, a negative pairStart or pairLength,
 * pairStart + pairLength > targetLength, pairStrand > 1.  Then the flat envelope of SetPairs with its messages ("... create
 * a new batch"): an empty query or an empty window, and under EDLIB_TASK_PATH the limits named there.  numPairs == 0 is
 * valid.
 * Every refusal is decided on the host from the lengths alone, before either batch changes, and leaves `pairs` as it
 * was: its previous pairs, the views the caller still holds, the results of its next Run.  Behind that point only a device
 * error can fail the call; it leaves `pairs` without pairs, as a failed SetPairs does.
 * The config of `pairs` and its additionalEqualities are its own and need not match those of `windows`; its alphabet is
 * the census of the gathered target bytes, as for any streamed set.
 * What crosses the link is the offsets and the tuples (about 25 bytes a pair); the host reads no byte of a sequence. */
EDLIB_API int edlibAmdBatchPairsSetWindows(EdlibAmdBatch* pairs, EdlibAmdBatch* windows,
    const int* pairQuery, const int* pairStart, const int* pairLength,
    const unsigned char* pairStrand /* NULL: all forward */, int numPairs);

/* The same from a READ batch (start locations and CIGARs for the reads a distance Run mapped, without the windows or the
 * reverse complements being made on the host): the query of pair i is read pairQuery[i] of `reads` -- its
 * edlibAmdReverseComplement where pairStrand[i] == 1 -- and its target is target[pairStart[i] .. pairStart[i] +
 * pairLength[i]) of the target of `reads`.  Afterwards `pairs` is exactly the batch edlibAmdBatchPairsSetPairs would have
 * made over these pairs materialised: everything that call keeps and resets this one keeps and resets, and Run, Results,
 * ResultsFlat, ResultsView, CigarView and Stats follow as there.  Returns 0, or non-zero with edlibAmdLastError().
 * The tuples are the caller's own: the first hit of a read, any other end location, a run of a hit-list batch, a padded
 * window.  For a read of m bases with HW distance d and first end location e >= 0, the window
 * [max(0, e - m - d + 1), e] gives the first start, the first end and the alignment of the whole-target HW / PATH answer,
 * shifted by the window's start (DESIGN.md 4b "Pairs from a read batch").
 * The bytes are copied: when the call returns `pairs` depends on nothing in `reads`, which may be run or destroyed.
 * `reads` is not changed in any way a caller can observe.
 * `pairs` is a batch of edlibAmdBatchCreatePairs in any state SetPairs accepts.  `reads` is a batch of
 * edlibAmdBatchCreateShared, ...SharedBothStrands or ...SharedHits in any state after Create (any number of Runs, none
 * included), with reads of any length and route, over any alphabet and mode: the source is the raw bytes of its target and
 * its query pool, so the 16-symbol limit of SetWindows does not apply.  Strand 1 of a both-strand batch reads the reverse
 * complement the batch made at Create; from the other two kinds it is reversed and complemented on the fly.
 * Refused, with this function and the reason named: a NULL handle; another kind of batch on either side (for `reads`: a
 * pair batch and a cross, self, occurrence or window batch); batches on different devices; numPairs < 0; a NULL
 * pairQuery, pairStart or pairLength with a positive count (a NULL pairStrand is all forward).  Per pair, the first
 * offender named with its values: pairQuery outside [0, numQueries) of `reads`, a negative pairStart or pairLength,
 * pairStart + pairLength > targetLength, pairStrand > 1.  Then the flat envelope of SetPairs with its messages: an empty
 * query or window, a query above 1,024 bases, a window above 65,536, and under EDLIB_TASK_PATH the limits named there.
 * numPairs == 0 is valid.  Every refusal is decided on the host from the lengths alone and leaves `pairs` as it was.
 * Behind that point only a device error can fail the call; it leaves `pairs` without pairs, as a failed SetPairs does. */
EDLIB_API int edlibAmdBatchPairsSetSharedWindows(EdlibAmdBatch* pairs, EdlibAmdBatch* reads,
    const int* pairQuery, const int* pairStart, const int* pairLength,
    const unsigned char* pairStrand /* NULL: all forward */, int numPairs);

/* The same from a CROSS or SELF batch (start locations and paths for the cells a cross batch found, the alignments of the
 * pairs within k of a self batch, without a sequence being sliced on the host or uploaded again): the query of pair i is
 * query pairQuery[i] of `cross` -- its edlibAmdReverseComplement where pairStrand[i] == 1 -- and its target is
 * target pairTarget[i] [pairStart[i] .. pairStart[i] + pairLength[i]), in the coordinates of that target; pairStart and
 * pairLength both NULL: every pair takes its whole target.  Over a self batch "query" and "target" are both sequences of
 * the one set, and any (i, j) is allowed, not only i < j.  Afterwards `pairs` is exactly the batch
 * edlibAmdBatchPairsSetPairs would have made over these pairs materialised: everything that call keeps and resets this
 * one keeps and resets, and Run, Results, ResultsFlat, ResultsView, CigarView and Stats follow as there.  Returns 0, or
 * non-zero with edlibAmdLastError().
 * The tuples are the caller's own: rows of EdlibAmdCrossHits, cells of the matrix, best hits, runs of an occurrence list,
 * pairs of EdlibAmdSelfHits.  For a cell of HW distance d and first end location e >= 0 of a query of m bases, the window
 * [max(0, e - m - d + 1), e] of its target gives the first start, the first end and the alignment of the whole-target
 * HW / PATH answer, shifted by the window's start; SHW: [0, e]; NW: the whole target (DESIGN.md 4b "Pairs from a cross
 * batch").
 * The bytes are copied: when the call returns `pairs` depends on nothing in `cross`, which may be given new targets, run
 * or destroyed.  `cross` is not changed in any way a caller can observe: its views, its next Run and its Stats stay.
 * `pairs` is a batch of edlibAmdBatchCreatePairs in any state SetPairs accepts.  `cross` is a batch of
 * edlibAmdBatchCreateCross, ...CrossHits, ...CrossOccurrences, ...CrossBothStrands, ...CrossHitsBothStrands,
 * ...CreateSelf, ...SelfHits, ...SelfBothStrands or ...SelfHitsBothStrands in any state after Create or after a
 * successful edlibAmdBatchCrossSetTargets (any number of Runs, none included).  Target bytes come from its resident 4-bit
 * pack and its code -> byte table (up to 16 symbols, bytes >= 128 included), query bytes from its resident query pool:
 * strand 1 of a both-strand batch reads the reverse complement the batch made at Create, from the other kinds it is
 * reversed and complemented on the fly.  A query of any length the flat envelope takes (up to 1,024 bases) may be named,
 * those above 256 bases that the cross kernel does not scan included.
 * Refused, with this function and the reason named: a NULL handle ("null pair batch", "null cross batch"); another kind
 * of batch on either side; batches on different devices; a batch left without targets by a failed SetTargets;
 * numPairs < 0; a NULL pairQuery or pairTarget with a positive count; exactly one of pairStart and pairLength NULL (a
 * NULL pairStrand is all forward).  Per pair, the first offender named with its values: a query or target index out of
 * range, a negative pairStart or pairLength, pairStart + pairLength beyond that target's length, pairStrand > 1, and a
 * target that is not in the pack -- one that ran through an internal session at Create because it has more than 65,536
 * bases or because the union alphabet exceeds 16 symbols, or any sequence of a self set outside the kernel's envelope:
 * materialise those pairs and use edlibAmdBatchPairsSetPairs.  Then the flat envelope of SetPairs with its messages: an
 * empty query or window, a query above 1,024 bases, and under EDLIB_TASK_PATH the limits named there.  numPairs == 0 is
 * valid.  Every refusal is decided on the host from the lengths alone, before either batch changes, and leaves `pairs` as
 * it was.  Behind that point only a device error can fail the call; it leaves `pairs` without pairs, as a failed SetPairs
 * does. */
EDLIB_API int edlibAmdBatchPairsSetCells(EdlibAmdBatch* pairs, EdlibAmdBatch* cross,
    const int* pairQuery, const int* pairTarget,
    const int* pairStart, const int* pairLength,        /* both NULL: every pair takes its whole target */
    const unsigned char* pairStrand /* NULL: all forward */, int numPairs);

/* edlibFreeAlignResult() over results[0..n) (one call instead of n for binding languages). */
EDLIB_API void edlibAmdFreeResults(EdlibAlignResult* results, int n);

/* Releases the process-wide cache of device / pinned blocks and idle streams the library keeps between calls. */
EDLIB_API void edlibAmdTrim(void);

/* Counters of the last Run.  The struct GROWS AT ITS END between versions of this library (wide_retries came last) and
 * edlibAmdBatchStats() writes all of it: this additive surface is versioned with the library, not frozen like edlib.h --
 * build clients against the header of the library they load. */
typedef struct {
    double run_ms;          /* HIP-event time of the whole last Run on its stream           */
    double scan_ms;         /* HIP-event time of the dominant scan kernel(s) in that Run     */
    int scan_launches;      /* number of scan-kernel launches in that Run                    */
    long long cells;        /* sum over units of queryLength * targetLength (GCUPS numerator)*/
    long long word_steps;   /* 32-row word-column updates the scan kernels executed          */
    long long algo_bytes;   /* algorithmic bytes: target+query+Peq+results    */
    int path;               /* bit 0 reads-per-lane kernel, bit 1 block-per-lane kernel, bit 2 piece filter (long HW reads), bit 3 cross kernel, bit 4 (value 16) window kernel */
    int overflow_units;     /* units whose end-location list needed the exact second pass    */
    int wide_retries;       /* launches of the many-wave kernel that gave up (not resident together / stalled) and were run again with one slot per unit */
} EdlibAmdBatchStats;

EDLIB_API int edlibAmdBatchStats(EdlibAmdBatch* batch, EdlibAmdBatchStats* out);
EDLIB_API void edlibAmdBatchDestroy(EdlibAmdBatch* batch);

#ifdef __cplusplus
}
#endif
#endif /* EDLIB_AMD_H */
