// engine_lanes.hpp -- the engines that put one query per lane over a packed target: cross batches with their self mode
// (engine_cross.hip, engine_self.hip) and window batches (engine_windows.hip).  LaneEngine (engine_lanes.hip) is what
// they keep alike: the resident query pool and packed target, the Peq buffers of a word group, the frame of a Run, the
// internal sessions of the units outside the kernels' envelope, and the pinned parts a view fetches.
#pragma once
#include "engine.hpp"

#include <initializer_list>

namespace edlib_amd {

// (PinnedPart: common.hpp)
struct WantedPart { int asked; PinnedPart* part; const void* dev; size_t bytes; };

// 65,536 as the messages of setTargets and setUnits write it

// The pairs of an internal pair Batch: the bytes of every pair replicated, query and target
struct PairPool {
    std::vector<char> qp, tp;
    std::vector<long long> qo = std::vector<long long>(1, 0), to = std::vector<long long>(1, 0);
    long long size() const { return (long long)qo.size() - 1; }
    void add(const char* q, long long qn, bool reverse, const char* t, long long tn);   // reverse: q's reverse complement
    int init(Batch& b, const EdlibAlignConfig& cfg, int device);
};

class LaneEngine {
public:
    EdlibAmdBatchStats stats{};

protected:
    // what every word group has: its query slots and their Peq rows (the engines' own groups extend it)
    struct LaneGroup {
        int words = 0, slots = 0;
        long long wordSteps = 0;                  // word-steps of what its scan takes
        DevBuf<int> d_perm, d_qlen, d_kinit, d_alpha;          // per query slot
        DevBuf<uint32_t> d_peq;
    };
    EdlibAlignConfig cfg_{};
    std::vector<EdlibEqualityPair> eqs_;
    int device_ = 0, nq_ = 0, syms_ = 4;
    hipStream_t stream_ = nullptr;
    Tables tab_;
    DevBuf<uint8_t> d_qpool_;
    DevBuf<long long> d_qoff_, d_tdw_;
    DevBuf<uint16_t> d_eqtbl_;
    DevBuf<uint32_t> d_presence_, d_tpk_;
    DevBuf<int> d_tperm_;
    DevBuf<int> d_best_;
    DevBuf<unsigned long long> d_bkey_;
    // results of the internal sessions on their way into the engine's arrays
    DevBuf<long long> d_cells_; DevBuf<int> d_vals_; PinBuf h_vals_;
    Event evScan0_, evScan1_;
    PinnedPart best_;
    bool haveRun_ = false;

    void closeStream();                           // the destructors': the members die behind the stream's work
    int openStream();                             // the stream and the scan events (the device is current)
    // the query pool (rebased) with its offsets, plain or as both strands of every query made on the device, and the tables
    int uploadQueries(const char* queries, const std::vector<long long>& qoff, bool strands);
    // the sequences order[i] (of lengths len[i]) of a device pool as 4-bit codes, back to back from dword 0
    int packTargets(const uint8_t* d_pool, const long long* d_off, const std::vector<int>& order, const std::vector<int>& len);
    // the same from the caller's memory: the raw pool is only needed by the pack
    int packHostTargets(const char* pool, const std::vector<long long>& off, const std::vector<int>& order,
                        const std::vector<int>& len);
    int allocGroup(LaneGroup& g, const std::vector<int>& perm);      // slots = perm's; the Peq buffers, perm uploaded
    int buildPeq(LaneGroup& g);
    // a Run's share of the engine's kernel: the Peq rows of every group, then scan() between the two scan events
    template <typename Groups, typename Scan>
    int scanRun(Groups& groups, unsigned pathBit, Scan&& scan) {
        if (groups.empty()) return 0;
        for (auto& g : groups)
            if (buildPeq(*g)) return 1;
        EDLIB_AMD_HIP(hipEventRecord(evScan0_.e, stream_));
        if (scan()) return 1;
        EDLIB_AMD_HIP(hipEventRecord(evScan1_.e, stream_));
        stats.path |= pathBit;
        return 0;
    }
    int beginRun(hipError_t guardStatus, std::initializer_list<PinnedPart*> parts);
    int endRun(std::chrono::steady_clock::time_point t0, bool scanned);
    int fetchParts(std::initializer_list<WantedPart> wants);         // a view's: the parts asked for are in pinned memory
    // (editDistance, numLocations, first end location) of the n units of an internal session's last run
    int readCells(Batch& b, size_t n, int* vals, const char* engine);
    // wordSteps = false: edlib_amd.h defines a self batch's word_steps as the kernel's pairs only
    void addSessionStats(Batch& b, bool wordSteps);
};

// Every query against every target (engine_cross.hip, DESIGN.md "Cross batches"): DISTANCE only, results as a
// target-major matrix and best hits, both made on the device.  Cells inside the cross kernel's envelope run on it; each
// other target runs through an internal shared-target Batch over all queries, longer queries against the rest through
// one internal pair Batch, and their results are scattered into the matrix.
// A hit-list batch (hits: k >= 0) keeps no matrix: the scan appends the cells within k to a list, the internal sessions'
// cells within k are appended behind them, and the list is sorted on the device into CSR order (per target, ascending
// query) and reduced to the same best hits.
// An occurrence batch (occ; HW, k >= 0, queries up to 256 bases; DESIGN.md §4h "Occurrence batches") is a hit-list batch
// whose list holds every maximal run of columns within k of every cell (five ints a run) instead of one record a cell:
// the scan appends closed runs, each target outside the kernel's envelope runs all queries through one internal hit-list
// shared-target Batch whose runs are re-keyed and appended behind them, and the list is sorted into CSR order by
// (target, query, firstEnd).  It keeps no best hits.
// A both-strand batch (strands) scans every query and its reverse complement (made on the device at init)
// as the mates of neighbouring slots; a cell is the better strand's record (resolve_strands) and a strand byte beside it.
// Its internal shared-target sessions are both-strand batches, its pair session holds both strands of every long query.
// A self batch (initSelf; engine_self.hip, DESIGN.md §4h "Self batches") is one set against itself, NW only: every
// unordered pair once, as a condensed vector or an i < j hit list, and the nearest other sequence of each.  nq_ = nt_ = n,
// the packed targets, the Peq build, the hit list and its finish are the cross batch's own.  On both strands (initSelf's
// strands) a pair is the better of its two sequences as they are and of the lower-indexed one's reverse complement
// against the other, with a strand byte per pair, per hit and per nearest partner.
class CrossBatch : public LaneEngine {
public:
    ~CrossBatch() { closeStream(); }
    int init(const char* queries, const long long* qoff, int nq, const char* targets, const long long* toff, int nt,
             EdlibAlignConfig cfg, int device, bool hits = false, bool strands = false, bool occ = false);
    int initSelf(const char* seqs, const long long* off, int n, EdlibAlignConfig cfg, int device, bool hits,
                 bool strands = false);
    // A hit-list self batch whose pair (i, j) exists only where groups[i] == groups[j] (DESIGN.md §4h "Grouped self
    // batches"): one strand, k >= 0; every view reports what a hit-list self batch over each group alone would
    int initSelfGrouped(const char* seqs, const long long* off, int n, const int* groups, EdlibAlignConfig cfg, int device);
    // Another target set for the resident queries (DESIGN.md §4h "Streamed targets"): prepared on the device into fresh
    // buffers and swapped in once it is known to lie inside the kernel's envelope; a refusal leaves the batch as it was
    int setTargets(const char* targets, const long long* toff, int nt);
    int run();
    int selfView(int what, EdlibAmdSelfView* out);
    int selfHitsView(EdlibAmdSelfHits* out);
    int selfStrandsView(int what, EdlibAmdSelfStrands* out);
    // The connected components of the pairs within maxDistance (< 0: the batch's k) of the last Run, labelled on the device
    // from the finished hit list or the condensed vector as they lie there (DESIGN.md §4h "Components"); any number of
    // times per Run.  A refusal leaves the batch and its other views as they were
    int selfComponents(int maxDistance, int what, EdlibAmdSelfComponents* out);
    // The K nearest other sequences of every sequence (self batches) / nearest queries of every target (cross batches)
    // within maxDistance (< 0: every reported distance) of the last Run, selected on the device from the results as they lie there
    // (DESIGN.md §4h "Neighbours"); any number of times per Run.  A refusal leaves the batch and its other views as they were
    int selfNeighbors(int K, int maxDistance, EdlibAmdNeighbors* out);
    int crossNeighbors(int K, int maxDistance, EdlibAmdNeighbors* out);
    bool isSelf() const { return self_; }
    int view(int what, EdlibAmdCrossView* out);
    int hitsView(EdlibAmdCrossHits* out);
    int strandsView(int what, EdlibAmdCrossStrands* out);
    int occurrencesView(EdlibAmdCrossOccurrences* out);
    bool bothStrands() const { return strands_; }
    bool isOccurrences() const { return occ_; }
    int device() const { return device_; }
    // What a pair batch gathers its pairs from (edlibAmdBatchPairsSetCells, `fn` in the messages): the resident query pool
    // and the pack of the targets the kernel takes, with the host's lengths of every query and target and which targets
    // are in the pack.  Waits for the batch's stream (Create and SetTargets prepare asynchronously) and makes, once per
    // target set, the place of every target in the pack's order.  1 with the error set for a batch a failed SetTargets
    // left without targets.  Nothing a caller can observe changes.
    int gatherSource(const char* fn, CellSource& out);

private:
    struct Group : LaneGroup {                    // slots: whole tiles, padded with -1
        int qt = 64, tiles = 0, ysplit = 1;       // wordSteps: of its scanned cells (NW, k >= 0: inside the length window)
        // self batches: the rank of every slot, and the work items (query tile, first target tile, trips) of its launch
        // (grouped self batches: d_end, one past the last rank of every slot's group)
        DevBuf<int> d_rank, d_items, d_end;
        int numItems = 0;
        int syms = 0;                             // Peq rows per word its buffers were allocated for
    };
    int nt_ = 0;
    size_t cells_ = 0;
    std::vector<std::unique_ptr<Group>> groups_;
    // the queries as init found them: their lengths, and those of each word count sorted by length (index = words); the
    // longest decides whether the batch takes setTargets
    std::vector<int> qlen_;
    std::vector<std::vector<int>> wordQueries_;
    long long qbytes_ = 0;
    int maxQlen_ = 0, longestQuery_ = -1;
    bool noTargets_ = false;                      // a setTargets failed on the device after it had begun to swap
    PinBuf h_census_;
    // The target-dependent shape of every word group over the numSorted_ targets on the kernel: choose_qt, tiles, ysplit,
    // wordSteps, the padded slot permutation.  colsBelow[L] (L <= kCrossMaxTarget + 1): columns of the targets shorter
    // than L.  A group's buffers are made again only where its tile or syms_ changed; no targets: no groups.
    int shapeGroups(const std::vector<long long>& colsBelow);
    // a target set being prepared on the device (prepareTargets), not yet the batch's (adoptTargets): the raw pool and
    // offsets, scratch, and what takes the place of d_tpk_ / d_tdw_ / d_tperm_ / d_tlen_
    struct TargetPrep {
        DevBuf<uint8_t> raw, tmp, tlut;
        DevBuf<long long> offIn, offR, dw, tdw;
        DevBuf<uint32_t> pres, len, idx, tpk;
        DevBuf<int> tlen, tperm;
    };
    int prepareTargets(const char* targets, const long long* toff, int nt, long long dwords, TargetPrep& p, Tables& tab);
    int adoptTargets(TargetPrep& p, int nt);
    int sizeResults();                            // the result buffers of nq_ x nt_ cells, made or grown
    int noResults();                              // the views': sets the error of a batch that has not run (or has no targets)
    int numSorted_ = 0;                           // targets on the cross kernel
    // gatherSource's: the length of every target and whether it is in the pack (init, initSelf and setTargets keep them;
    // a self batch's are its sequences', which are its queries too), and the inverse of d_tperm_ on the device, made at
    // the first call after a target set arrived
    std::vector<int> tlenHost_;
    std::vector<uint8_t> inPack_;
    DevBuf<int> d_place_;
    bool placeReady_ = false;
    long long sortedCols_ = 0;                    // their columns
    DevBuf<int> d_tlen_;
    DevBuf<int> d_mat_;                           // [3][nt][nq]: editDistance, numLocations, endLocation
    // d_best_: [3][nt] then [3][nq]
    DevBuf<CrossBest2> d_partial_;
    int targetChunk_ = 1024;
    // cells of the other engines: each out-of-envelope target's column (shared Batch), the long queries' cells (pair Batch)
    std::vector<std::unique_ptr<Batch>> outShared_;
    std::vector<int> outTargets_;
    std::unique_ptr<Batch> longPairs_;
    std::vector<long long> longCells_;
    long long otherCells_ = 0;
    PinnedPart mat_;
    // hit-list batches: nothing here scales with numQueries x numTargets; the list starts at max(2^20, nq + nt) entries
    // and grows to the count of a Run that overflowed it (that Run scans again)
    // (hit_list.hpp): three planes as appended (editDistance, numLocations, endLocation), [4][n] in CSR order with the
    // query in front, offsets [nt + 1]; both strands: a strand byte per entry
    bool hits_ = false;
    // occurrence batches (hits_ is set too): an entry is a run, five planes (firstEnd, lastEnd, editDistance, endLocation,
    // numLocations), [6][n] finished; no best hits
    bool occ_ = false;
    HitListBuffers hitList_;
    int sizeHitList(long long minCap);            // the list configured for this kind of batch, of nt_ rows
    std::vector<long long> otherCellIdx_;         // cells of the internal sessions (t * nq + q), host side
    HitRows otherHits_;                           // their cells within k (occurrence batches: their runs) of the last Run
    // both strands: a strand byte (bit 0 reverse complement, bit 1 the other strand reaches the same distance) per cell
    // [nt][nq] or per hit, and per best hit [nt] then [nq]
    bool strands_ = false;
    DevBuf<uint8_t> d_smat_, d_sbest_, d_svals_;
    PinnedPart cellStrand_, bestStrand_;
    PinBuf h_svals_;
    // self batches: d_mat_ is the condensed vector [n (n - 1) / 2] (cells_), longPairs_ the i < j pairs outside the
    // kernel's envelope; selfOther_ the keys (i << 32) | j of the pairs answered off the kernel -- first the selfEmpty_
    // pairs with an empty sequence (distance: the other's length), then the pairs of longPairs_
    bool self_ = false;
    bool grouped_ = false;                        // initSelfGrouped: only the pairs inside a group exist (cells_ counts them)
    std::vector<unsigned long long> selfOther_;
    std::vector<int> selfEmptyVal_;
    DevBuf<int> d_near_;                          // [3][n]: nearest, nearestDistance, secondDistance
    PinnedPart near_;
    // components: one block carved by SelfComponentsBuffers, made at the first call and kept; comp_ is fetched at every call
    DevBuf<int> d_comp_;
    PinnedPart comp_;
    // neighbours: the block carved by NeighborsBuffers and, for a self hit list, the one carved by NeighborsMirror, made
    // at the first call and kept (grow-only); nbr_ is fetched at every call
    DevBuf<int> d_nbr_;
    DevBuf<uint8_t> d_mirror_;
    PinnedPart nbr_;
    // `who` names the call in the messages; the checks every neighbours call shares, then level = maxDistance, -1 where it is < 0
    int neighborsLevel(const char* who, int K, int maxDistance, int* level);
    // the selection over `src` into d_nbr_, the block back in one copy, `out` filled
    int selectNeighbors(const NeighborsSource& src, int K, int level, EdlibAmdNeighbors* out);
    // both-strand self batches: d_smat_ is the condensed strand vector, cellStrand_ its (or the hit list's) pinned part;
    // d_sbest_ is [2 n] for the hits finish, then [n] the strand byte of every nearest partner (bestStrand_); a pair of
    // selfOther_ behind the empty ones is the pairs 2c (forward) and 2c + 1 (the lower index reverse-complemented) of
    // longPairs_
    int runSelf();
    int gather(Batch& b, size_t n, int* vals, uint8_t* sbytes);
    int runOccurrenceSessions();                  // the internal hit-list sessions' runs into otherHits_
    int scanGroups();
    int finishHits();                             // the list settled (otherHits_ behind the scan's) and finished on the device
};
// tile width of a word group: the lanes a tile shape leaves idle decide it (engine_cross.hip)
int choose_qt(long long nq, long long nt, int minQt = 1);

// Units over one resident target (engine_windows.hip, DESIGN.md "Window batches"): unit u is query unitQuery[u] against
// the window [unitStart[u], unitStart[u] + unitLength[u]) of the target, DISTANCE only, a cross batch's cell contract per
// unit and the best unit per query, both made on the device.  The target is packed once and every query's Peq is built
// once per Run whatever the number of units that name them; units outside the window kernel's envelope (query above 256
// bases, window above 65,536 columns, more than 16 target symbols) run through one internal pair Batch over slices
// materialised at Create and are scattered into the unit arrays.
// setUnits (DESIGN.md §4i "Streamed units") passes other queries and units through the resident batch: the target, its
// pack and its tables stay, the set is checked on the host and grouped, ordered and given Peq slots on the device
// (window_units.hip), the way init prepares a list that lies inside the kernel's envelope.
class WindowBatch : public LaneEngine {
public:
    ~WindowBatch() { closeStream(); }
    // unitStrand (NULL: all forward): 1 = the unit is the reverse complement of its query; the query pool then holds both
    // strands of every query (made on the device) and a Peq slot goes to each (query, strand) a kernel unit names
    int init(const char* queries, const long long* qoff, int nq, const char* target, int targetLength,
             const int* unitQuery, const int* unitStart, const int* unitLength, const unsigned char* unitStrand,
             int numUnits, EdlibAlignConfig cfg, int device);
    // Other queries and units for the resident target (DESIGN.md §4i "Streamed units"): checked on the host in one pass
    // over the offsets and one over the units, then uploaded as they are and grouped, ordered and given Peq slots on the
    // device; a refusal leaves the batch as it was
    int setUnits(const char* queries, const long long* qoff, int nq, const int* unitQuery, const int* unitStart,
                 const int* unitLength, const unsigned char* unitStrand, int numUnits);
    int run();
    int view(int what, EdlibAmdWindowView* out);
    int device() const { return device_; }
    // What a pair batch gathers its pairs from (edlibAmdBatchPairsSetWindows, `fn` in the messages): the resident query
    // pool and target pack of a set that was prepared on the device.  1 with the error set where nothing is resident: a
    // target of more than 16 symbols, a Create that took the host route, a setUnits that failed on the device.  The batch
    // is not changed.
    int gatherSource(const char* fn, WindowSource& out) const;

private:
    struct Group : LaneGroup {                    // slots: the (query, strand) entries its units name, unpadded
        int numSorted = 0;                        // wordSteps: of its scanned units (not the empty or the NW-skipped ones)
        // per unit, sorted by window length; of a set prepared on the device these and d_perm are views into prep_
        DevBuf<int> d_uslot, d_ustart, d_ulen, d_uperm;
    };
    // what the host's pass over a unit list finds
    struct UnitCensus {
        bool stranded = false;                    // a unit names a reverse complement
        bool inside = true;                       // every unit lies inside the window kernel's envelope
        int longUnit = -1;                        // the first window above 65,536 columns
        long long cells = 0;
        int units[kCrossMaxQueryWords + 1] = {};              // per word group
        long long wordSteps[kCrossMaxQueryWords + 1] = {};
    };
    // the unit checks of Create and SetUnits in one pass; 0 with the census filled, or 1 with the first bad unit named
    static int checkUnits(const long long* qoff, int nq, int targetLength, const int* unitQuery, const int* unitStart,
                          const int* unitLength, const unsigned char* unitStrand, int nu, int mode, int k, UnitCensus& c);
    // the device buffers of a prepared set: the uploads, the scratch of window_units.hip and its results, all grow-only
    struct UnitPrep {
        DevBuf<uint8_t> raw, strand, named, tmp;
        DevBuf<long long> offIn;
        DevBuf<int> ustart, ulen;                 // as the caller gave them (the unit queries are d_uq_)
        DevBuf<uint32_t> ukey, uval, ukeyS, ekey, eval, ekeyS;
        DevBuf<int> slotOf, ent, bound;
        DevBuf<int> suslot, sustart, sulen, superm;            // the scan's arrays, every group's back to back
        PinBuf h_bound;
    } prep_;
    // the queries and units of a checked set made the batch's on the device (Create and SetUnits); a device error leaves
    // the batch without units (noUnits_)
    int prepareUnits(const char* queries, const long long* qoff, int nq, const int* unitQuery, const int* unitStart,
                     const int* unitLength, const unsigned char* unitStrand, int nu, const UnitCensus& c);
    int noResults();                              // Run's and the views': the error of a batch without units or without a Run
    bool noUnits_ = false;                        // a setUnits failed on the device after it had begun to change the batch
    // of the set prepareUnits made last (none: a Create on the host route): the host's copy of the queries' offsets as the
    // caller gave them (any base: a gathered set is planned from their differences), and whether the pool holds both strands
    bool onDevice_ = false, stranded_ = false;
    std::vector<long long> h_qoff_;
    int nu_ = 0, targetLength_ = 0;
    std::unique_ptr<Group> groupOf_[kCrossMaxQueryWords + 1];  // the group of every word count, kept for its buffers
    std::vector<Group*> groups_;                  // those that have units
    DevBuf<int> d_uq_;                            // [nu] query of every unit (the best reduction)
    DevBuf<int> d_units_;                         // [3][nu]: editDistance, numLocations, endLocation
    // d_best_: [3][nq], d_bkey_: [2][nq]
    // units outside the kernel's envelope: one pair Batch over their materialised slices
    std::unique_ptr<Batch> pairs_;
    std::vector<long long> pairUnits_;
    PinnedPart units_;
};

}  // namespace edlib_amd
