// engine.hpp -- host side of the engine: batches of alignment units resident in
// HBM, scheduled onto the two kernel families.  This is the re-expression of the
// orchestration in reference edlibAlign() (edlib.cpp:146-301) for a batch.
#pragma once
#include "../../include/edlib_amd.h"
#include "common.hpp"
#include "pair_kernels.hpp"
#include "lanepair.hpp"
#include "reads_kernels.hpp"
#include "cross_kernels.hpp"
#include "window_kernels.hpp"
#include "strands.hpp"
#include "flat_pairs_prepare.hpp"
#include "pairs_gather.hpp"

#include <chrono>
#include <deque>
#include <functional>
#include <memory>
#include <vector>

namespace edlib_amd {

// Byte-level tables shared by every unit of a batch:
// the target alphabet and the equality relation of EqualityDefinition
// (edlib.cpp:63-94) expressed on raw bytes.
struct Tables {
    uint8_t tlut[256];        // target byte -> symbol id (first appearance order)
    uint8_t idToByte[256];    // symbol id -> byte
    int sigmaT = 0;           // number of distinct target bytes
    uint32_t presence[8];     // bitset of the target bytes
    uint16_t eqtbl[256];      // query byte -> 16-bit set of the (first 16) target symbols it equals
    std::vector<uint8_t> eq8; // [256*256] eq8[q*256+t] = 1 if bytes q and t are equal; EMPTY = identity
};

// A unit handed to the block-per-lane kernels (host mirror of PairDesc).
struct UnitSpec {
    long long qoff; int qlen; int qstep;
    long long toff; int tlen; int tstep;
    int kinit;
    int skip = 0;      // HW target segments: leading warm-up columns whose scores are not recorded
    int band = 0;      // SHW: scan only the diagonals [-kinit, kinit] (a cell within kinit of the origin's diagonal has |i - j| <= kinit);
                       // HW: only [-kinit, (tlen - qlen) + 2 kinit] (an alignment within kinit starts in [0, tlen - qlen + kinit])
};

struct SolveOut {
    std::vector<int> score, count, last;
    std::vector<long long> posStart;      // [units+1] into posFlat (exact, complete lists)
    std::vector<int> posFlat;
    // op strings stay where the D2H put them (pinned staging, one block per chunk); units point into it
    std::vector<const uint8_t*> opsPtr;
    std::vector<int> opsLen;
    std::vector<std::shared_ptr<PinBuf>> opsBufs;
    void reset(size_t n) {                // n units without an answer
        score.assign(n, -1); count.assign(n, 0); last.assign(n, -1);
        posStart.assign(n + 1, 0); posFlat.clear();
        opsPtr.assign(n, nullptr); opsLen.assign(n, 0); opsBufs.clear();
    }
};

// Units answered by several solves, put back in unit order: unit i takes entry q of `from` (score, count, last, its slice
// of posFlat; no op strings), a unit nothing was taken for has no answer.  The SolveOuts outlive write().
struct Assembler {
    struct Pick { const SolveOut* from = nullptr; size_t q = 0; };
    std::vector<Pick> pick;
    explicit Assembler(size_t n) : pick(n) {}
    void take(size_t i, const SolveOut& from, size_t q) { pick[i].from = &from; pick[i].q = q; }
    void write(SolveOut& out) const {
        out.reset(pick.size());
        for (size_t i = 0; i < pick.size(); ++i) {
            if (const SolveOut* p = pick[i].from) {
                const size_t q = pick[i].q;
                out.score[i] = p->score[q]; out.count[i] = p->count[q]; out.last[i] = p->last[q];
                out.posFlat.insert(out.posFlat.end(), p->posFlat.begin() + p->posStart[q], p->posFlat.begin() + p->posStart[q + 1]);
            }
            out.posStart[i + 1] = (long long)out.posFlat.size();
        }
    }
};

// What the threshold ladder of banded semi-global units (Batch::solveBanded) leaves to the mode
struct BandLadder {
    int mode;
    bool (*enter)(const UnitSpec& u, long long& K);                          // does the unit climb at all, and from which K
    UnitSpec (*level)(const UnitSpec& u, long long K);                       // the unit as level K <= u.kinit scans it
    bool (*final)(const UnitSpec& u, const UnitSpec& level, int score);      // is that level's answer the unit's
};

// Op string of one job: a view into a staging block, or an owned concatenation (Hirschberg pieces).
struct OpsOut {
    const uint8_t* p = nullptr;
    int len = 0;
    std::vector<uint8_t> own;
};

// Location lists of a unit: almost always one or two entries, so they live inside the result record (a
// std::vector here was two malloc / free pairs per read: most of what LOC / PATH cost on a read batch); longer
// lists move to the heap.  24 bytes: the host side of LOC / PATH is bound by walking these records.
class LocList {
public:
    LocList() = default;
    ~LocList() { delete big_; }
    LocList(const LocList& o) { append(o.data(), o.n_); }
    LocList& operator=(const LocList& o) { if (this != &o) { clear(); append(o.data(), o.n_); } return *this; }
    LocList(LocList&& o) noexcept : n_(o.n_), big_(o.big_) { in_[0] = o.in_[0]; in_[1] = o.in_[1]; o.n_ = 0; o.big_ = nullptr; }
    LocList& operator=(LocList&& o) noexcept {
        if (this != &o) { delete big_; n_ = o.n_; big_ = o.big_; in_[0] = o.in_[0]; in_[1] = o.in_[1]; o.n_ = 0; o.big_ = nullptr; }
        return *this;
    }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    const int* data() const { return n_ <= kInline ? in_ : big_->data(); }
    int* data() { return n_ <= kInline ? in_ : big_->data(); }
    int operator[](size_t i) const { return data()[i]; }
    int& operator[](size_t i) { return data()[i]; }
    void clear() { n_ = 0; }                              // keeps the heap block (records are recycled across runs)
    void push_back(int v) { append(&v, 1); }
    void append(const int* p, size_t c) {
        const size_t nn = n_ + c;
        if (nn <= kInline) { for (size_t i = 0; i < c; ++i) in_[n_ + i] = p[i]; }
        else {
            if (!big_) big_ = new std::vector<int>();
            if (n_ <= kInline) big_->assign(in_, in_ + n_);
            big_->insert(big_->end(), p, p + c);
        }
        n_ = (uint32_t)nn;
    }
    void assign(size_t c, int v) {
        n_ = 0;
        if (c <= kInline) { for (size_t i = 0; i < c; ++i) in_[i] = v; }
        else { if (!big_) big_ = new std::vector<int>(); big_->assign(c, v); }
        n_ = (uint32_t)c;
    }
private:
    static const uint32_t kInline = 2;
    uint32_t n_ = 0;
    int in_[kInline];
    std::vector<int>* big_ = nullptr;
};

// Per-unit result assembled on the host before it is marshalled into
// EdlibAlignResult (malloc'd arrays) by results().
struct UnitResult {
    int status = EDLIB_STATUS_OK;
    int editDistance = -1;
    int alphabetLength = 0;
    bool hasEnds = false, hasStarts = false, hasAlignment = false;
    LocList ends, starts;
    const uint8_t* opsView = nullptr;         // op string: a view into a staging block (or an owned string) the batch keeps alive
    int opsViewLen = 0;
};

struct Lap;                        // (below)
struct ViewLayout; struct ViewVar; // engine_flat.hip

// The host's one pass over the offsets of a pair set (engine_flat.hip: planFlat): whether the set lies inside the flat
// envelope -- if not, the first pair outside it and why -- and the reductions its layout needs.  No sequence byte is read.
struct FlatPlan {
    enum Why { kOk = 0, kBadQueryOffsets, kBadTargetOffsets, kEmptyQuery, kEmptyTarget, kLongQuery, kLongTarget, kPathBlocks,
               kHirschberg, kStoreCap, kOpsCap };
    Why why = kOk; int who = -1;                  // the first offending pair
    int n = 0, maxBlocks = 0, maxWords = 0;
    long long qbytes = 0, tbytes = 0, cells = 0, lens = 0, totalBlocks = 0;
    long long opBytes = 0, store4 = 0, store32 = 0;   // PATH: op slots; entries of the 4-lane ring stores, of the ring32 stores
    long long chunkMax32 = 0;                         // ... and of the largest chunk of the ring32 NW store
    std::vector<int> cuts;                            // first units of those chunks, then n
};

class Batch {
public:
    virtual ~Batch();
    // sequences are copied to the device here; nothing of the caller's memory is retained
    int init(const char* queries, const long long* qoff, int n,
             const char* targets, const long long* toff, int numTargets,   // numTargets == 1: shared
             EdlibAlignConfig cfg, int device, bool bothStrands = false,    // bothStrands (shared only): n reads, 2n units
             bool hits = false,                                             // hits (shared only): a hit-list read batch
             bool pairs = false);                                           // made by edlibAmdBatchCreatePairs (one pair is shared, too)
    // another pair set through a resident pair batch (edlibAmdBatchPairsSetPairs; engine_flat.hip "streamed pairs")
    int setPairs(const char* queries, const long long* qoff, const char* targets, const long long* toff, int n);
    // the same with the pairs named as (query, strand, window) tuples over a window batch and gathered from its resident
    // pools on the device (edlibAmdBatchPairsSetWindows; engine_flat.hip "pairs from a window batch")
    // (fn: the caller's name in the messages -- edlibAmdBatchPairsSetSharedWindows gathers from a read batch the same way)
    int setWindows(const char* fn, const WindowSource& src, const int* pairQuery, const int* pairStart, const int* pairLength,
                   const unsigned char* pairStrand, int n);
    // what a read batch (not a pair batch) lends to that gather: its query pool and its raw target, behind a wait for
    // init's upload (engine_flat.hip "pairs from a window batch")
    int gatherSource(const char* fn, WindowSource& out);
    // the same with the pairs named as (query, target, window, strand) tuples over a cross or self batch and gathered from
    // its query pool and its pack of targets (edlibAmdBatchPairsSetCells; engine_flat.hip "pairs from a cross batch");
    // pairStart and pairLength both null: every pair takes its whole target
    int setCells(const char* fn, const CellSource& src, const int* pairQuery, const int* pairTarget, const int* pairStart,
                 const int* pairLength, const unsigned char* pairStrand, int n);
    bool isPairs() const { return pairsKind_; }
    int device() const { return device_; }
    bool isBothStrands() const { return strands_; }
    int run();
    int runImpl();
    int results(EdlibAlignResult* out);
    int resultsFlat(int* status, int* editDistance, int* numLocations, int* alphabetLength, long long* locOffsets,
                    int** endLocations, int** startLocations, long long* alnOffsets, unsigned char** alignment);
    int resultsView(EdlibAmdResultsView* out);
    int cigarView(int format, const char** chars, const long long** offsets);
    int strandView(EdlibAmdStrandView* out);
    int hitsView(EdlibAmdReadHits* out);
    bool isHits() const { return hits_; }
    EdlibAmdBatchStats stats{};
    void finishStats();          // fills the fields of `stats` that cost a walk over the records (algo_bytes)

private:
    // ---- configuration
    EdlibAlignConfig cfg_{};
    std::vector<EdlibEqualityPair> eqs_;
    int device_ = 0;
    bool shared_ = false;
    bool pairsKind_ = false;                     // created by edlibAmdBatchCreatePairs: takes setPairs
    bool noPairs_ = false;                       // a setPairs failed on the device: no Run, no views until one succeeds
    int noResults(const char* who);              // the error of a view that has nothing to show
    int n_ = 0;
    std::vector<long long> qoff_, toff_;
    // ---- both strands: unit 2i is read i, unit 2i + 1 its reverse complement (made on the device at init);
    // the caller sees n_ / 2 units, each the record of unit 2i + strand[i]
    bool strands_ = false;
    PinBuf h_strand_;                            // [outN()] strand, then [outN()] bothStrands, of the last run
    int outN() const { return strands_ ? n_ / 2 : n_; }
    int unitOf(int u) const { return strands_ ? 2 * u + h_strand_.p[u] : u; }
    void setStrand(int read, int code) { h_strand_.p[read] = (uint8_t)(code & kStrandReverse); h_strand_.p[outN() + read] = (code & kStrandBoth) ? 1 : 0; }
    int resolveStrandsOnHost(std::vector<UnitResult>& res);      // the mate pairs outside the read groups, from their records
    int hostStrandCounts_[4] = {0, 0, 0, 0};                     // of the pairs resolveStrandsOnHost decided in the last run
    int strandCounts(int counts[4]);                             // forward, reverse, both, none of the last run (debug line)
    Tables tab_;
    hipStream_t stream_ = nullptr;
    Event evRun0_, evRun1_, evA_, evB_;           // evB_: the side stream's alphabet kernel is done

    // ---- resident inputs
    DevBuf<uint8_t> d_in_;                       // offsets + small tables (+ small sequence pools) in one block
    PinBuf h_in_;                                // its pinned staging (kept until the batch dies: the copy is asynchronous)
    DevBuf<uint8_t> d_qpool_, d_tpool_, d_tlut_, d_idToByte_, d_eq8_;
    DevBuf<uint16_t> d_eqtbl_;   // views into d_in_ unless large
    hipError_t uploadEq8();
    DevBuf<uint32_t> d_presence_;
    DevBuf<long long> d_qoff_, d_toff_;

    // ---- unit classification (phase 1)
    std::vector<int> emptyUnits_, readUnits_, pairUnits_;
    std::vector<int> longUnits_;                 // HW queries above 256 rows against the shared target (long_reads.hip)
    std::vector<int> pairNow_;                   // pair units of the current run: pairUnits_ + what the piece filter handed back
    // ---- a run: beginRun, the phases in runImpl()'s order, endRun (engine.hip); a hit-list Run has the same frame
    int beginRun(hipError_t guardStatus);
    int enqueueWordSteps();
    int endRun();
    void resetRecords(std::vector<UnitResult>& res);
    void answerEmptyUnits(std::vector<UnitResult>& res);
    int runFlatPhase(std::vector<UnitResult>& res, Lap& lap);
    int runLongReads(std::vector<UnitResult>& res, Lap& lap);
    int runPairPhase(std::vector<UnitResult>& res, Lap& lap);
    int runStartsPhase(std::vector<UnitResult>& res, Lap& lap);
    int runPathsPhase(std::vector<UnitResult>& res, Lap& lap);
    void startStats();                           // algo_bytes where the run knows it; finishStats() is its other half
    bool flatDone_ = false;                      // this run stayed on the flat pair path: no records, no later phases

    // ---- reads-per-lane path
    struct ReadGroup {
        int nwords = 0, nslots = 0, numSegments = 1, segLen = 0, warm = 0, mMin = 0, mMax = 0;   // mMin, mMax: the shortest and the longest query (0: not known)
        std::vector<int> perm;                 // slot -> unit (or -1)
        DevBuf<int> d_perm, d_qlen, d_kinit, d_alphaExtra, d_segBest, d_segCnt, d_segPos;
        DevBuf<int> d_best, d_total, d_pos, d_flags;
        DevBuf<uint32_t> d_peq;
        bool zeroCopy = false; PinBuf hostOut;   // small groups: d_best / d_total / d_alphaExtra / d_flags / d_pos are views into pinned host memory
        // exact second pass of the last run: overflowing slots, their offsets into d_ovfPool
        std::vector<int> ovfSlots; std::vector<long long> ovfOff; DevBuf<int> d_ovfPool;
        // segment records of the k-doubling levels (engine_reads.hip), kept from run to run; after a run whose last level
        // ran (lvValid) they hold that level: lvMap = its lanes' slots (ascending), lvS segments, lvCap positions per segment
        DevBuf<int> d_lvMap, d_lvBest, d_lvCnt, d_lvPos; std::vector<int> lvMap; int lvS = 0, lvCap = 0; bool lvValid = false;
        DevBuf<int> d_list;                    // [nslots + 1] a slot list compacted on the device, then its length
        int nreal = -1;                        // slots that hold a unit (counted when first needed)
        // both strands: the slots s and s ^ 1 hold a read and its reverse complement (the groups made at init only);
        // d_win[p]: what the pair in the slots 2p, 2p + 1 reports (strands.hpp), decided after the levels of a run
        bool mates = false; DevBuf<int> d_win;
    };
    static constexpr int kLastLevelCap = 16;   // positions per (lane, segment) of the last level = the slot's own 16
    int listOpenSlots(ReadGroup& g, int kDone, std::vector<int>& out);
    DevBuf<uint8_t> d_selTmp_;                 // rocPRIM select scratch
    std::vector<std::unique_ptr<ReadGroup>> groups_;
    DevBuf<uint32_t> d_tpk_, d_trows_;
    DevBuf<unsigned long long> d_wordSteps_;
    PinBuf h_wordSteps_; bool wordStepsPending_ = false;
    DevBuf<unsigned long long> d_ringSteps_; PinBuf h_ringSteps_; bool ringStepsUsed_ = false;   // live word-steps of the ring kernels of a run
    unsigned long long* ringStepsCounter();
    bool banded_ = false;        // HW groups use the Ukkonen-banded kernel with k-doubling
    int syms_ = 4;               // Peq rows per word of the reads kernels: target symbols rounded up to 4, 8 or 16
    int packTarget();
    int runReads();                                   // device work only; results stay in HBM
    int makeGroup(const std::vector<int>& units, int words, std::unique_ptr<ReadGroup>& g, long long oneRoundWaves = 0);
    int runGroupScans(ReadGroup& g, bool fullOnly);
    int runGroupExact(ReadGroup& g);
    int collectGroup(ReadGroup& g, std::vector<UnitResult>& res);
    // ---- exact k-mer seed filter in place of the banded first pass (reads_seed.hip)
    int seedThreshold(const ReadGroup& g, bool fullOnly) const;   // k_f of the group, -1: the group takes the banded pass
    int buildSeedIndex();                                         // buckets of the shared target (every run, after packTarget)
    int runSeedPass(ReadGroup& g, int k);                         // pass 1 at threshold k, hand-backs through the banded kernel
    DevBuf<uint32_t> d_seedCnt_, d_seedOff_, d_seedPos_;          // [4^12 + 1] counts, [4^12 + 1] bucket offsets, [T] positions
    DevBuf<uint8_t> d_seedTmp_;                                   // rocPRIM scan scratch
    // ---- hit-list read batches (reads_hits.hip): every maximal run of columns scoring <= k, HW / DISTANCE,
    // reads up to 256 bases.  A Run is Peq rows, the HITS scans of every group (seeded where seedThreshold() allows k), and the
    // finish on the device; nothing else of runImpl() runs.  The list (hit_list.hpp) starts at max(2^20, n_) runs and grows to
    // the count of a Run that overflowed it (that Run scans again).
    bool hits_ = false, hitsHaveRun_ = false;
    HitListBuffers hitList_;
    HitRows hostHits_;                                            // the empty reads' hits, answered on the host
    DevBuf<int> d_hitSlotUnit_;                                   // slot -> unit, -1 = padding: all groups' slots, then one per empty unit
    DevBuf<long long> d_hitTotal_;                                // hits of the stitched list
    int runReadHits();                                            // the whole Run of such a batch
    int scanGroupHits(ReadGroup& g, int slotBase);                // one group's runs appended to the list
    int hitsScanBanded(ReadGroup& g, int slotBase, const int* d_slotmap, int nlanes, int numSegments, int segLen, int warm);
    // ---- long HW queries: piece filter on the reads-per-lane kernel + window verification on kernel W (long_reads.hip)
    struct Piece { long long off; int len; int thr; };           // rows [off, off + len) of the query pool, threshold of its scan
    int scanPieces(const std::vector<Piece>& pieces, bool filter, std::vector<std::pair<int, int>>* cand,
                   std::vector<uint8_t>* overflow, std::vector<int>* best);
    int solveLongReads(std::vector<UnitResult>& res, std::vector<int>& fallback);
    bool filterScan_ = false;
    // strips of taller queries on the full-height lane kernel, chained through HBM (long_reads.hip: solveTallFull)
    struct ChainArgs { const uint32_t* in = nullptr; uint32_t* out = nullptr; const int* src = nullptr; int inLanes = 0, blocks = 0; const int* rowBase = nullptr; };
    ChainArgs chain_;
    int solveTallFull(const std::vector<int>& units, std::vector<UnitResult>& res, std::vector<int>& handBack);
    int collectReads(std::vector<UnitResult>& res);   // D2H + result semantics (lazy for TASK_DISTANCE)
    bool readsCollected_ = true;
    int scanGroup(ReadGroup& g, int mode, const int* d_slotmap, int nlanes, int kcap, const int* d_kinit,
                  int numSegments, int segLen, int warm, int* segBest, int* segCnt, int* segPos, int cap,
                  const long long* posOff, const int* posCap, bool unbanded = false,
                  unsigned long long* wordSteps = nullptr, const uint32_t* peqDense = nullptr,
                  const int* qlenDense = nullptr, int peqBottom = 0, int* liveBest = nullptr,
                  const Segment* segTable = nullptr, long long tableCols = 0);   // segTable: its segments (with numSegments), tableCols: columns a lane walks

    // ---- block-per-lane path
    DevBuf<PairDesc> d_descs_;
    DevBuf<unsigned long long> d_peq64_;
    DevBuf<StoreEntry> d_store_;
    DevBuf<int> d_aux_, d_out3_, d_outScore_, d_outCount_, d_outLast_, d_posPool_, d_opsLen_, d_alpha_;   // d_out{Score,Count,Last}_: views into d_out3_
    DevBuf<uint8_t> d_ops_;
    DevBuf<long long> d_opsOff_;
    // ring = 0: unbanded strips (any mode).  ring = 4 / 16 / 64: NW inside Ukkonen's band for threshold
    // UnitSpec::kinit on rings of that many lanes (exact iff score <= kinit); the caller guarantees that
    // the band fits (kinit <= ring_max_k(ring), or the unit has at most `ring` blocks)
    // ringH = 2 / 4 (ring 16, no path): ring lanes of 2 / 4 vertically adjacent blocks, band limit ring_max_k(16, ringH)
    int solve(int mode, bool wantPositions, bool wantPath, const std::vector<UnitSpec>& units, SolveOut& out,
              int ring = 0, int ringH = 1);
    int solveChunk(int mode, bool wantPositions, bool wantPath, const std::vector<UnitSpec>& units,
                   size_t a, size_t b, SolveOut& out, int ring, int ringH);
    // ---- one unit on many waves (wide_kernels.hip): `ring` = kWide in solve() / solveChunk().  NW: the band of threshold
    // UnitSpec::kinit, any width (exact iff score <= kinit); SHW / HW: the pipelined strips.  Distances / positions only.
    static const int kWide = -1;
    static const int kRing32 = -2;                // solve(): storing NW scans on 16-lane rings of 32-row words (the caller checked ring32_fits)
    bool ring32_fits(const std::vector<UnitSpec>& units, size_t a, size_t b, int G) const;
    DevBuf<unsigned long long> d_wide_; DevBuf<unsigned> d_wabort_; PinBuf h_wabort_;
    int wideCap_ = -1;                           // resident waves of the wide kernel on this device
    struct WidePlan { int slots = 1; size_t perLaunch = 1; };
    int planWide(int mode, PairDesc* descs, size_t n, WidePlan& plan);      // slots per unit, units per launch; assigns auxOff
    int launchWide(int mode, const PairScanArgs& a, const PairDesc* hostDescs, size_t n, const WidePlan& plan);
    int checkWide();                             // after the stream is idle: 0 fine, 2 a launch gave up (run the units again: one slot each), 1 error.  Releases the device's wide gate.
    bool wideSerial_ = false;                    // this run's wide launches take one slot per unit (after an aborted launch)
    bool wideGateHeld_ = false;                  // this batch holds its device's wide gate (launchWide .. checkWide)
    void wideGateRelease();
    // NW distance of long units as two half scans that meet in the middle (forward over the left half of the target,
    // reverse over the right half, both inside the band of UnitSpec::kinit): out[4 u ..] = {min, split row, left, right};
    // exact iff min <= kinit
    int solveWideSplit(const std::vector<UnitSpec>& units, std::vector<int>& out, int ring = 0);     // ring > 0: the halves on lane rings
    // what the distance phase of this run already knows about a piece's first split (solveWideSplit): the path phase
    // does not scan the two halves again
    struct KnownSplit { long long qoff; int m; long long toff; int T; int score; int row, left, right; };
    std::vector<KnownSplit> knownSplits_;
    // NW distances by threshold levels on rings of 4, 16, 64 lanes, then unbanded (the reference's
    // k-doubling, edlib.cpp:197-217, with thresholds chosen for the hardware)
    // paths != null (TASK_PATH, every unit below the 1 MiB rule): the levels run with the column store and the traceback, so
    // that a unit's first successful level is also its path (one scan instead of the distance scan + the storing scan)
    int solveGlobalDistances(const std::vector<UnitSpec>& units, std::vector<int>& score, std::vector<OpsOut>* paths = nullptr);
    // SHW / HW units: short queries packed on 4- and 16-lane rings, the rest on the strips
    int solveSemiGlobal(int mode, bool wantPositions, const std::vector<UnitSpec>& units, SolveOut& out);
    int solveSemiGlobalUnits(int mode, bool wantPositions, const std::vector<UnitSpec>& units, SolveOut& out);
    // SHW / HW inside the band of a threshold: levels K, 4 K, 16 K ... like the NW distances, by the mode's BandLadder
    int solveBanded(const BandLadder& ladder, bool wantPositions, const std::vector<UnitSpec>& units, SolveOut& out);
    // alphabetLength of the empty / pair units: launched on a side stream before phase 1, collected after it
    int alphabetLengthsBegin(hipEvent_t after = nullptr);      // after: the side stream also waits for this event
    bool alphaDeferred_ = false;
    int alphabetLengthsEnd(std::vector<UnitResult>& res);
    std::vector<int> alphaUnits_; bool alphaOnHost_ = false, alphaPending_ = false; long long alphaBytes_ = 0;
    hipStream_t side_ = nullptr;
    DevBuf<int> d_alphaIdx_, d_alphaOut_; PinBuf alphaPin_;
    // linear-space paths (reference obtainAlignmentHirschberg, edlib.cpp:1231-1396)
    struct PathPiece { long long qoff; int m; long long toff; int T; int score; };
    int hirschbergLevel(const std::vector<PathPiece>& big, std::vector<int>& splitRow,
                        std::vector<int>& leftScore, std::vector<int>& rightScore);
    int solvePaths(const std::vector<PathPiece>& jobs, std::vector<OpsOut>& opsOut, std::vector<int>& status);
    std::vector<std::shared_ptr<PinBuf>> opsKeep_;      // staging blocks the last run's op views point into
    std::deque<std::vector<uint8_t>> opsOwned_;         // op strings assembled on the host (Hirschberg pieces, empty windows)

    int qlen(int u) const { return (int)(qoff_[u + 1] - qoff_[u]); }
    long long tbase(int u) const { return shared_ ? toff_[0] : toff_[u]; }
    int tlen(int u) const { return shared_ ? (int)(toff_[1] - toff_[0]) : (int)(toff_[u + 1] - toff_[u]); }

    void scanTimerStart();
    void scanTimerStop();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> scanEvents_;
    size_t scanEventsUsed_ = 0;

    std::vector<UnitResult> results_, work_;     // last run's records / the next run's (ping-pong: no reallocation per run)
    std::vector<UnitSpec> startUnits_; std::vector<std::pair<int, int>> startWhere_; std::vector<int> live_;
    bool haveResults_ = false;
    long long algoBase_ = -1;     // algorithmic bytes of the batch while its results are still on the device
    bool algoDirty_ = false;
    // per-unit scratch of the pair path, kept across runs (fresh multi-megabyte vectors are mmap + page faults + munmap)
    std::vector<int> pairSpecsFor_;              // the pair units pairSpecs_ was built for
    std::vector<UnitSpec> pairSpecs_, selScratch_; std::vector<size_t> whoScratch_; std::vector<int> lvlScratch_, scoreMain_;
    SolveOut soMain_, soLevel_;
    // a ladder level that takes every unit of a big pair batch (engine_pairs.hip): compact specs resident per batch,
    // descriptors written by a kernel, the Peq of all units built on a third stream while the divergence probe runs
    int pairSpecsVersion_ = 0, levelSpecsVersion_ = -1, shapeVersion_ = -1, alphaIsPairsVersion_ = -1;
    bool alphaIsPairs_ = false;
    struct PairShape { size_t minBlocks = 0, maxBlocks = 0; int minLenLo = 0, minLenHi = 0, maxDiff = 0; } shape_;   // of pairSpecs_
    long long levelPeqWords_ = 0;
    bool levelAllReady_ = false;
    PinBuf h_levelSpecs_, h_levelScore_;
    DevBuf<LevelSpec> d_levelSpecs_;
    DevBuf<PairDesc> d_descsAll_;
    DevBuf<unsigned long long> d_peqAll_;
    hipStream_t aux_ = nullptr;
    Event evLevelIn_, evLevelPeq_;
    int prepareLevelAll(const std::vector<UnitSpec>& units);
    std::function<void()> whileScanning_;        // host work of the run that does not depend on the scan: done behind the level's launch
    int runLevelAll(const std::vector<UnitSpec>& units, int ring, int ringH, int ringBlocks, int cap, int kcap, int nbMax);
    // ---- the lane-per-pair level of big NW distance batches over at most four target symbols (lanepair.hpp):
    // a lane owns a unit, the band narrows with the scores.  The units' packed layout is resident like the offset arrays;
    // a run packs the sequences (query / target bit planes; alphabetLength counted on the way) beside the divergence probe
    // and scans every unit at the probe's threshold; what that leaves open climbs the rings.
    int laneSpecsVersion_ = -1;
    long long lanePlaneWords_ = -1, laneTgtWords_ = 0;
    bool laneReady_ = false;
    PinBuf h_laneUnits_, h_laneScore_;
    DevBuf<lanepair::LaneUnit> d_laneUnits_;
    DevBuf<lanepair::Plane2> d_lanePlanes_;
    DevBuf<lanepair::Tgt2> d_laneTgts_;
    DevBuf<int> d_laneFlags_, d_laneScore_;
    Event evLanePack_;
    int alphabetBuffers();
    int prepareLaneLevel(const std::vector<UnitSpec>& units);
    int runLaneLevel(const std::vector<UnitSpec>& units, double rate, int kcap, int W);
    std::vector<OpsOut> fusedOps_;
    // ---- flat pair path (every unit a pair of at most 16 blocks): descriptors built once and resident, a run is Peq
    // build + ONE ring scan + an overflow census, results stay in HBM until results() (like the reads path).
    // flat LOC / PATH (round 4): start locations and paths of a flat batch are found and kept on the device as well.
    // HW starts: one reverse prefix scan per end location, descriptors written by a kernel from the phase-1 results;
    // paths: one storing scan per unit over its window + the traceback into resident op slots.  What the fixed layouts
    // cannot hold (more than 16 end locations, a band level that fails) makes the run fall back to the general path.
    bool flatPairs_ = false, pairsCollected_ = true, lastRunFlat_ = false;
    // What prepareFlat decided about the resident set, on the host; a default-constructed value is "no flat set"
    struct FlatSet {
        int scanMode = EDLIB_MODE_NW;           // of the config (flatScanMode)
        int ring = 0;                           // lanes of the phase-1 ring
        bool ring32 = false;                    // storing scans and walks on rings of 32-row words (ring32_kernels.hip)
        int maxBlocks = 0, maxWords = 0;
        bool starts = false, paths = false, nwStore = false;
        std::vector<int> chunkStart;            // ring32 NW store: unit ranges whose store fits 32-bit offsets (one range = the usual case)
        long long wordSteps = 0;                // word-steps inside the bands of one run over the flat descriptors
        long long revPeqBase = 0, opsTotal = 0;
        size_t startCap = 0;
    } flat_;
    // exact lists of the last run's overflowing units (the lists themselves, and d_flatOvfAt_ / d_flatOvfOff_, are on the
    // device: the collection reads them there while `unit` is not empty)
    struct FlatOverflow {
        std::vector<int> unit; std::vector<long long> off{0};
        void clear() { unit.clear(); off.assign(1, 0); }
    } flatOvf_;
    void dropFlatSet() { flatPairs_ = false; flat_ = FlatSet{}; flatOvf_.clear(); }
    int flatG32_ = 8;                          // lanes of the rings of 32-row words
    // the config's mode as the kernels number it (NW, SHW or HW); -1: it has no flat form
    int flatScanMode() const {
        const int mode = (int)cfg_.mode;
        return (mode == EDLIB_MODE_HW || mode == EDLIB_MODE_SHW) ? mode : (mode == EDLIB_MODE_NW ? mode : -1);
    }
    FlatShape flatShape() const;
    DevBuf<PairDesc> d_flatDescs_;
    DevBuf<int> d_flatOut3_, d_flatPos_, d_flatCensus_;
    PinBuf h_flatCensus_;
    int flatCensus() const { return *reinterpret_cast<const int*>(h_flatCensus_.p); }   // behind the wait that follows enqueueFlatCensus
    DevBuf<int> d_flatOvfAt_, d_flatOvfPool_; DevBuf<long long> d_flatOvfOff_;
    DevBuf<PairDesc> d_flatRevDescs_, d_flatStartDescs_, d_flatPathDescs_;
    DevBuf<int> d_flatSlotOf_, d_flatStartOut3_, d_flatStartsOut_, d_flatPathOut3_, d_flatOpsLen_;
    DevBuf<long long> d_flatOpsOff_, d_flatStoreBase_;
    DevBuf<uint8_t> d_flatOps_, d_tsym_;
    void planFlat(const long long* qoff, const long long* toff, int n, bool sharedTarget, FlatPlan& plan,
                  std::vector<long long>* qout, std::vector<long long>* tout) const;
    int initFlatPairs();
    int prepareFlat(const FlatPlan& plan, bool census);      // the set's layout, made on the device: Create and a streamed set
    DevBuf<long long> d_flatPrep_; DevBuf<uint8_t> d_flatPrepTmp_; DevBuf<int> d_flatCuts_;
    struct FlatPrepOut { uint32_t presence[8]; unsigned long long steps[2]; };      // what prepareFlat brings back
    DevBuf<FlatPrepOut> d_flatPrepOut_; PinBuf h_flatPrepOut_;
    // a streamed set (setPairs, setWindows) takes the place of the batch's (replaceFlatSet): the refusal of a plan that
    // failed, what the batch drops before the set changes, the device's share with `fill` -- the pairs' bytes into the two
    // pools, on the stream -- in its middle
    enum { kSetRefused = 1, kSetLost = 2 };                  // replaceFlatSet: the batch is as it was; it has no pairs
    int replaceFlatSet(const char* fn, const FlatPlan& plan, std::vector<long long>& qnew, std::vector<long long>& tnew,
                       const std::function<int()>& fill);
    void refuseFlat(const char* fn, const FlatPlan& plan, long long m, long long T) const;
    int dropForStreamedSet(const FlatPlan& plan, std::vector<long long>& qnew, std::vector<long long>& tnew);
    int loadFlatSet(const FlatPlan& plan, const std::function<int()>& fill);
    DevBuf<int> d_gatherTuples_;                             // setWindows: pairQuery [n], pairStart [n], pairStrand (bytes)
                                                             // setCells: the 64-bit bases [n], pairQuery, pairTarget, pairStart [n], pairStrand
    std::vector<long long> gatherQoff_;                      // gatherSource of a both-strand batch: the reads' n + 1 offsets
    DevBuf<uint8_t> d_tabs_; PinBuf h_tabs_;                 // tlut, idToByte, eqtbl of a streamed set
    // a Run (runPairsFlat) and its phases; every scan takes its arguments from flatScanArgs
    int runPairsFlat(bool& fellBack);
    PairScanArgs flatScanArgs(const PairDesc* descs, int count, int* out3, size_t out3Stride) const;
    int flatStoreAndWalk(const PairDesc* descs, int* out3, int u0, int count);
    template <class Count> int enqueueFlatCensus(Count count);
    int runFlatNwPaths(bool& fellBack);
    int runFlatOverflowPass(const PairScanArgs& phase1);
    int runFlatStarts(bool& fellBack);
    int runFlatPaths();
    int collectPairsFlat(std::vector<UnitResult>& res);
    bool readsViewOnDevice() const;               // a DISTANCE run over read groups only: its view is made by flat_results.hip
    int buildReadsView();
    bool deferReadsReset_ = false;                // this run blanks the recycled records of reads-path units where it fills them (collectGroup)
    bool deferReset_ = false;                     // ... and of pair units where it fills them (runPairPhase)
    // the caller-facing arrays of the last run: made on the device for a flat batch (buildFlatView), from the records otherwise
    DevBuf<uint8_t> d_view_; PinBuf h_view_, h_viewVar_; bool viewReady_ = false;     // host: per-unit fields + offsets / locations + op bytes
    EdlibAmdResultsView view_{};
    const uint8_t* viewAlnDev_ = nullptr; const long long* viewAlnOffDev_ = nullptr;     // the dense op bytes on the device (CIGARs)
    std::vector<int> viewInts_; std::vector<long long> viewOffs_; std::vector<uint8_t> viewOps_;   // host-made view of a general batch
    int buildFlatView();
    int buildHostView();
    int fetchViewHead(const ViewLayout& L, long long capLoc, long long capAln, const char* who, ViewVar& var);
    // CIGAR strings of the last run (edlibAlignmentToCigar, edlib.cpp:303-350, over the batch): [0] extended, [1] standard
    struct CigarOut { bool ready = false; PinBuf chars, offs; std::vector<char> hostChars; std::vector<long long> hostOffs; const char* p = nullptr; const long long* off = nullptr; };
    CigarOut cigar_[2];
    DevBuf<long long> d_cigWork_; DevBuf<char> d_cigChars_, d_cigChars2_;
    bool cigarSticky_ = false;                   // a caller of this batch has asked for CIGARs: later collections make them while the op bytes travel
    Event evView_;
    int enqueueCigars(int f, const uint8_t* aln, const long long* alnOff, size_t cap, hipStream_t st);
    int fetchCigars(int f, hipStream_t st);
    int ensureCollected();                       // results of the last run that are still on the device -> results_
};

// single-pair convenience used by edlibAlign()
int align_one(const char* q, int qn, const char* t, int tn, EdlibAlignConfig cfg, EdlibAlignResult* out);
// one small pair in one kernel launch (one_pair.hip): 0 = answered, 1 = error, 2 = not handled here (take align_one)
int align_one_fused(const char* q, int qn, const char* t, int tn, EdlibAlignConfig cfg, EdlibAlignResult* out);

// EDLIB_AMD_DEBUG: host wall time between named points of a run (stderr)
struct Lap {
    bool on; std::chrono::steady_clock::time_point t;
    Lap() : on(getenv("EDLIB_AMD_DEBUG") != nullptr), t(std::chrono::steady_clock::now()) {}
    void operator()(const char* what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[edlib_amd] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// helpers shared by the translation units of the host side
static inline bool switched_off(const char* v) { return v && v[0] == '0'; }      // an environment switch set to "0..."
const int kMaxDevices = 16;                       // devices the process-wide caches and gates are kept for
const int kPosCap = 16;                           // end positions kept beside a pair unit's results (longer lists: exact second pass)
int peq_row_stride(long long nb);                 // row length of the LDS-resident Peq of the ring kernels
bool needs_hirschberg(int m, int T);              // the reference's 1 MiB rule (edlib.cpp:1188-1190)
void blank_record(UnitResult& r);
void finalize_global(UnitResult& r, int kcfg, int mode, int T, int score);
long long hw_band_rows(const UnitSpec& u, long long K);     // rows per column of the HW band of threshold K
// helpers shared by engine.hip and long_reads.hip
int roundup(int x, int q);
void plan_segments(int nlanes, int T, int mode, int warmFull, long long wantWaves, int& S, int& segLen, int& warm, int minSegCols = 4096);
// waves of the 24- / 32-word full-height lane kernels (24 / 32 KB of LDS rows each) the chip runs without two of them sharing
// a SIMD: one per SIMD of 256 CUs (swept in round 4: DESIGN.md 3c)
inline long long tall_round_waves() { return 1024; }
void finalize_semiglobal(UnitResult& r, int kcfg, int m, int best, const int* pos, long long npos);
// target alphabet and equality tables of a batch (engine.hip)
void build_tables(Tables& tab, const uint8_t* targets, long long totalTargetBytes, const EdlibEqualityPair* eqs, int neq);
// what every batch's init does alike (engine_lanes.hip); each keeps its own order of refusals
int check_device(int device);                     // 1 and the error text: no usable device, or `device` out of range
void keep_config(const EdlibAlignConfig& cfg, EdlibAlignConfig& kept, std::vector<EdlibEqualityPair>& eqs);   // kept points into eqs
int copy_offsets(const long long* in, int n, const char* what, std::vector<long long>& out);    // "bad <what> offsets"
std::string with_commas(long long v);                // thousands separators for the sizes a refusal names
inline int peq_syms(int sigmaT) { return sigmaT <= 4 ? 4 : (sigmaT <= 8 ? 8 : 16); }   // Peq rows per word: 4, 8 or 16

int device_count();
int host_threads(int cap);
int default_device();

}  // namespace edlib_amd
