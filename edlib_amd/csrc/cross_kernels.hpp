// cross_kernels.hpp -- launch interface of the cross kernels (every query against every target, DISTANCE only):
// the 4-bit target pack, the lane-per-cell scan, the best-hit reductions and the scatter of cells computed elsewhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hit_list.hpp"

namespace edlib_amd {

constexpr int kCrossMaxQueryWords = 8;          // queries up to 256 symbols (kernel A's word groups)
constexpr int kCrossMaxTarget = 65536;          // longer targets take the shared-target engine
constexpr int kCrossMaxSyms = 16;               // union target alphabet of the cross kernel

// Result of one cell from what its scan left: the rules of finalize_global / finalize_semiglobal (engine.hip), with the
// empty-sequence case of the reference (edlib.cpp:167-183) in front.  HW / SHW: best = smallest bottom-row score over the
// target columns, cnt = number of columns at it, first = the first of them (best > every threshold when n == 0).
// NW: best = score of the last column.
// NW with k >= 0: a cell whose lengths differ by more than k is above k without a scan (the reference's own early exit,
// edlib.cpp:744); the kernel skips the columns of such a cell and cross_cell_result() answers -1 for it.
__host__ __device__ inline bool cross_nw_outside(int mode, int kcfg, int m, int n)
{
    return mode == 0 && kcfg >= 0 && (m > n ? m - n : n - m) > kcfg;
}

__host__ __device__ inline void cross_cell_result(int mode, int kcfg, int m, int n, int best, int cnt, int first,
                                                  int& ed, int& nloc, int& end)
{
    if (m == 0 || n == 0) {
        if (mode == 0) { ed = m > n ? m : n; nloc = 1; end = n - 1; }
        else { ed = m; nloc = 1; end = -1; }
        return;
    }
    if (cross_nw_outside(mode, kcfg, m, n)) { ed = -1; nloc = 0; end = -1; return; }
    if (mode == 0) {
        if (kcfg >= 0 && best > kcfg) { ed = -1; nloc = 0; end = -1; }
        else { ed = best; nloc = 1; end = n - 1; }
        return;
    }
    // candidates score <= min(k, m): HW clamps k to m, SHW's best never exceeds m; the empty target prefix (-1) takes
    // part when the reference's padded last block sees it (W > 0)
    const int thr = (kcfg < 0 || kcfg > m) ? m : kcfg;
    const int W = ((m + 63) / 64) * 64 - m;
    const bool kAllowsM = (kcfg < 0 || kcfg >= m);
    if (best > thr) {
        if (W > 0 && kAllowsM) { ed = m; nloc = 1; end = -1; }
        else { ed = -1; nloc = 0; end = -1; }
        return;
    }
    const bool lead = W > 0 && best == m;
    ed = best;
    nloc = cnt + (lead ? 1 : 0);
    end = lead ? -1 : first;
}

// Best and second best of a row of distances (-1 = not within k): key = (distance << 32) | index, the smaller key wins,
// so ties go to the lowest index whatever the order of the reduction.  ~0 = none.
struct CrossBest2 { unsigned long long b, s; };

__device__ __forceinline__ unsigned long long cross_key(int ed, int idx)
{
    return ed < 0 ? ~0ull : (((unsigned long long)(uint32_t)ed << 32) | (uint32_t)idx);
}

__device__ __forceinline__ void best2_add(CrossBest2& r, const unsigned long long key)
{
    if (key < r.b) { r.s = r.b; r.b = key; }
    else if (key < r.s) r.s = key;
}

__device__ __forceinline__ void best2_merge(CrossBest2& r, const CrossBest2& o)
{
    if (o.b < r.b) { r.s = r.b < o.s ? r.b : o.s; r.b = o.b; }
    else { r.s = r.s < o.b ? r.s : o.b; }
}

__device__ __forceinline__ void best2_store(const CrossBest2& r, int* best, int* bestD, int* secondD, int i)
{
    best[i] = r.b == ~0ull ? -1 : (int)(uint32_t)r.b;
    bestD[i] = r.b == ~0ull ? -1 : (int)(r.b >> 32);
    secondD[i] = r.s == ~0ull ? -1 : (int)(r.s >> 32);
}

// What the scan of one query group needs.  The group's slots are tiles of `qt` queries; lane l of a wave takes query slot
// tile * qt + l % qt against sorted target tile * (64 / qt) + l / qt.
struct CrossScanArgs {
    const uint32_t* peq;        // the group's Peq, [slot / 64][S][NWD][slot % 64] (build_peq_reads_kernel)
    const int* qlen;            // [slots]
    const int* qperm;           // [slots] slot -> query index, -1 for a padding slot
    int qt;                     // queries per tile: 64, 32, ..., 1
    int numQueryTiles;
    const uint32_t* tpk;        // target pool, 4 bits per column, 8 columns per dword, each target from a dword boundary
    const long long* tdw;       // [numSorted] first dword of sorted target i
    const int* tlen;            // [numSorted]
    const int* tperm;           // [numSorted] sorted target -> target index
    int numSorted;
    int numQueries;             // row length of the matrix
    int kcfg;
    int* ed; int* nloc; int* end;   // [numTargets][numQueries] (dense batches)
    // hit-list batches: every cell whose editDistance is not -1 is appended (hit_list.hpp) as the key
    // (target << 32) | query and three planes: editDistance, numLocations, endLocation
    HitList hits;
    // both-strand batches (launch_scan_cross_strands): qperm = 2 * query + strand with mates in the slots s and s ^ 1, qt
    // even, numQueries the number of queries (not of slots); one strand byte (bit 0 reverse complement, bit 1 the other
    // strand reaches the same distance) per stored cell [numTargets][numQueries], per appended hit [hits.cap] in a hit list
    uint8_t* strand;
    // self batches (launch_scan_cross_self / launch_scan_cross_self_strands; DESIGN.md §4h "Self batches"): queries and targets are one set, the targets
    // in the order (length, index) -- a sequence's position there is its rank --, the query slots of a group in the same
    // order.  A lane scans cell (slot, ts) only where ts > qrank[slot]; block b takes work item b, the query tile
    // items[3b] against the target tiles [items[3b + 1], items[3b + 1] + items[3b + 2]).  ed is the condensed vector of
    // numQueries sequences (pair (i, j), i < j, at numQueries i - i (i + 1) / 2 + j - i - 1), a hit's key (i << 32) | j.
    // Both strands: qperm = 2 * sequence + strand, mates in the slots s and s ^ 1 with one qrank, a tile holds qt / 2
    // sequences; strand is [numPairs] in condensed order, [hits.cap] in a hit list.
    const int* qrank;           // [slots] rank of the slot's sequence, -1 for a padding slot
    const int* items;           // [3][numItems] as triples
    int numItems;
    // grouped self batches (launch_scan_cross_self_groups; DESIGN.md §4h "Grouped self batches"): the order is (group,
    // length, index), and a lane scans cell (slot, ts) only where qrank[slot] < ts < qend[slot]
    const int* qend;            // [slots] one past the last rank of the group of the slot's sequence, -1 for a padding slot
};

hipError_t launch_pack_cross_targets(const uint8_t* raw, const long long* toff, const int* tperm, const long long* tdw,
                                     int numSorted, const uint8_t* tlut, uint32_t* tpk, hipStream_t stream);
// nwords 1..8, syms 4 / 8 / 16, mode 0 NW / 1 SHW / 2 HW; ysplit: waves per query tile (each strides over target tiles);
// hits: append the cells within k to the hit list instead of writing the matrix
hipError_t launch_scan_cross(int nwords, int syms, int mode, bool hits, const CrossScanArgs& a, int ysplit,
                             hipStream_t stream);
// the same scan over both strands of every query (cross_kernels_strands.hip): the combined cell per mate pair
hipError_t launch_scan_cross_strands(int nwords, int syms, int mode, bool hits, const CrossScanArgs& a, int ysplit,
                                     hipStream_t stream);
// the occurrence scan (cross_kernels_occ.hip; HW, kcfg >= 0): every maximal run of columns scoring <= kcfg of every cell
// appended to a.hits as the key (target << 32) | query and five planes: its firstEnd, lastEnd, editDistance, endLocation,
// numLocations; a cell's runs are appended in ascending column order
hipError_t launch_scan_cross_occ(int nwords, int syms, const CrossScanArgs& a, int ysplit, hipStream_t stream);
// the self scan (cross_kernels_self.hip): NW only, one block per work item
hipError_t launch_scan_cross_self(int nwords, int syms, bool hits, const CrossScanArgs& a, hipStream_t stream);
// the self scan over both strands of the row sequence (cross_kernels_self_strands.hip): the combined pair per mate pair
hipError_t launch_scan_cross_self_strands(int nwords, int syms, bool hits, const CrossScanArgs& a, hipStream_t stream);
// the grouped self scan (cross_kernels_self_groups.hip): NW, hit list, one strand, one block per work item
hipError_t launch_scan_cross_self_groups(int nwords, int syms, const CrossScanArgs& a, hipStream_t stream);
// nearest other sequence of each of n sequences from the condensed vector: out [3][n] = nearest, nearestDistance,
// secondDistance (the key rule of CrossBest2 over all partners on either side of the triangle)
hipError_t launch_self_nearest_dense(const int* ed, int n, int* out, hipStream_t stream);
// the same from the best hits of a finished hit list (launch_cross_hits_finish with numQueries = numTargets = n and keys
// (i << 32) | j, i < j): best [3][n] over the partners above, then [3][n] over the partners below
hipError_t launch_self_nearest_hits(const int* best, int n, int* out, hipStream_t stream);
// out [n]: the strand byte of the pair (i, nearest[i]) from the condensed strand vector, 0 where nearest is -1
hipError_t launch_self_nearest_strand_dense(const uint8_t* pairStrand, const int* nearest, int n, uint8_t* out,
                                            hipStream_t stream);
// the same from a finished both-strand hit list: best as for launch_self_nearest_hits, bestStrand [n] over the partners
// above then [n] over the partners below
hipError_t launch_self_nearest_strand_hits(const int* best, const uint8_t* bestStrand, int n, uint8_t* out,
                                           hipStream_t stream);
// distances computed by other engines into the condensed vector: ed[cell[i]] = vals[i]
hipError_t launch_self_scatter(const long long* cell, const int* vals, long long n, int* ed, hipStream_t stream);
// the connected components of a self batch's pairs within a level (self_components.hip): views into one block of
// ints(n) ints -- first what travels, back to back: label [n], size [n], numComponents (and a pad), offsets [n + 1],
// members [n] (and a pad) -- then the work arrays
struct SelfComponentsBuffers {
    int *label, *size, *numComponents, *offsets, *members;
    int *parent, *count, *iota, *slabel, *flag, *rank;
    static size_t ints(int n);
    static SelfComponentsBuffers carve(int* base, int n);
};
// bytes of scratch the members' sort and scan need for n sequences
hipError_t self_components_scratch(int n, size_t* bytes);
// init, hook, flatten, sizes and (members) the grouping, enqueued on the stream.  The edges are the finished hit list's
// (cond == nullptr: the sorted keys (i << 32) | j, the partner and ed planes, [numHits] each) or the condensed vector's
// (cond), each where its distance d is 0 <= d and, with level >= 0, d <= level.  n = 0: nothing
hipError_t launch_self_components(const SelfComponentsBuffers& b, int n, const unsigned long long* skey, const int* partner,
                                  const int* ed, long long numHits, const int* cond, int level, bool members,
                                  void* scratch, size_t scratchBytes, hipStream_t stream);
// the K nearest neighbours of every row (neighbors.hip, DESIGN.md §4h "Neighbours").  Where a row's candidates lie:
//   kMatrix     row t is ed[t * rowLength ..], the index implicit (a dense cross batch: rowLength = numQueries)
//   kCondensed  row i is the n - 1 cells of the condensed vector `ed` that name i (a dense self batch: rowLength = n)
//   kCsr        row r is the entries [off[r], off[r + 1]) of the partner and distance planes; position[e] (nullptr: e
//               itself) is where entry e lies in its source, which is where its strand byte is
// strand (nullptr: none): the strand bytes by source position -- the cell of the matrix or of the condensed vector, or the
// position above
struct NeighborsSource {
    enum { kMatrix = 0, kCondensed = 1, kCsr = 2 };
    int kind, numRows, rowLength;
    const int* ed;
    const long long* off;
    const int* partner;
    const int* distance;
    const uint32_t* position;
    const uint8_t* strand;
};
// views into one block of ints(rows, K) ints, what travels back to back: count [rows], neighbor [rows][K],
// distance [rows][K], strand bytes [rows][K]
struct NeighborsBuffers {
    int *count, *neighbor, *distance;
    uint8_t* strand;
    static size_t ints(int rows, int K);
    static NeighborsBuffers carve(int* base, int rows, int K);
};
// the symmetric CSR of a self hit list (each pair under both its ends), views into one block of bytes(n, numHits) bytes
struct NeighborsMirror {
    long long* off;                         // [n + 1]
    int *degree, *cursor;                   // [n + 1], [n]
    int *partner, *distance;                // [2 numHits]
    uint32_t* position;                     // [2 numHits] the hit's place in the finished list
    static size_t bytes(int n, long long numHits);
    static NeighborsMirror carve(uint8_t* base, int n, long long numHits);
};
hipError_t neighbors_mirror_scratch(int n, size_t* bytes);       // of the scan over n + 1 degrees
// degree count, exclusive scan and scatter of the finished list (sorted keys (i << 32) | j, partner and ed planes)
hipError_t launch_neighbors_mirror(const NeighborsMirror& m, int n, const unsigned long long* skey, const int* partner,
                                   const int* ed, long long numHits, void* scratch, size_t scratchBytes, hipStream_t stream);
// a wave per row: the K (1..64) smallest keys (distance << 32) | index among the row's candidates whose distance d is
// 0 <= d and, with level >= 0, d <= level; -1 / -1 / 0 behind count[row]
hipError_t launch_neighbors_select(const NeighborsSource& s, int K, int level, const NeighborsBuffers& out, hipStream_t stream);
// per target over its queries (rows of the matrix) and per query over the targets (columns); out arrays are
// best index / best distance / second distance
hipError_t launch_cross_best(const int* ed, int numQueries, int numTargets,
                             int* bestQ, int* bestQD, int* secondQD, int* bestT, int* bestTD, int* secondTD,
                             CrossBest2* partial, int targetChunk, hipStream_t stream);
// out [numTargets] then [numQueries]: the strand byte of every best cell (0 where there is none)
hipError_t launch_cross_best_strands(const uint8_t* cellStrand, int numQueries, int numTargets, const int* bestQ,
                                     const int* bestT, uint8_t* out, hipStream_t stream);
// cells computed by other engines: ed / nloc / end of cell[i] (index into the matrix)
hipError_t launch_cross_scatter(const long long* cell, const int* vals, long long n, int* ed, int* nloc, int* end,
                                hipStream_t stream);
hipError_t launch_cross_scatter_bytes(const long long* cell, const uint8_t* vals, long long n, uint8_t* out,
                                      hipStream_t stream);

// ---- hit lists (cross_hits.hip), over a settled list (hit_list.hpp)
// The hits (three planes) into CSR order: sorted by key (target-major, ascending query inside a target), gathered into
// hl.out() [4][n] (query, editDistance, numLocations, endLocation), hl.off() [nt + 1] from the boundaries of the sorted
// keys; best hits per target and per query from the list into best ([3][nt] then [3][nq], the layout of
// launch_cross_best) through bkey ([2][nt + nq]).  Both-strand batches (bestStrand != NULL; the list carries a byte per
// entry): the strand byte travels with its hit into hl.byteOut, and bestStrand ([nt] then [nq]) is the byte of every
// best hit.
hipError_t launch_cross_hits_finish(HitListBuffers& hl, int numQueries, int numTargets, unsigned long long* bkey, int* best,
                                    uint8_t* bestStrand, hipStream_t stream);
// The runs of an occurrence batch (five planes) into CSR order: the same stable sort by key -- a cell's runs were
// appended in ascending column order, so they stay so behind it: (target, query, firstEnd) --, gathered into hl.out()
// [6][n] (query, firstEnd, lastEnd, editDistance, endLocation, numLocations), hl.off() [nt + 1] as above.
hipError_t launch_cross_occ_finish(HitListBuffers& hl, int numTargets, hipStream_t stream);

// ---- a target set prepared on the device (cross_targets.hip)
// temporary bytes of launch_cross_targets_prepare over n targets
hipError_t cross_targets_order_bytes(int n, size_t* bytes);
// From the raw pool and the caller's offsets offIn [n + 1] (any base, every length at most kCrossMaxTarget): the rebased
// offsets offR [n + 1], the presence set of the pool's bytes (8 dwords, zeroed here), the targets in the stable order
// (length, index) as tlen / tperm [n], and tdw [n], the first dword of every packed target in that order (the exclusive
// scan of ceil(length / 8)).  len, idx [n] and dw [n] are scratch.
hipError_t launch_cross_targets_prepare(const uint8_t* raw, const long long* offIn, int n, long long* offR,
                                        uint32_t* presence, uint32_t* len, uint32_t* idx, int* tlen, int* tperm,
                                        long long* dw, long long* tdw, void* tmp, size_t tmpBytes, hipStream_t stream);

}  // namespace edlib_amd
