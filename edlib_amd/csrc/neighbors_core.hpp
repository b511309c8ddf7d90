// neighbors_core.hpp -- the K nearest neighbours of every row of a self or cross batch (edlibAmdBatchSelfNeighbors,
// edlibAmdBatchCrossNeighbors, DESIGN.md §4h "Neighbours"): what does not need a wave.
//
// A candidate of a row is (distance, index); its key is (distance << 32) | index -- cross_key's rule, so the smaller key
// is the nearer candidate and ties go to the lower index.  An index occurs once in a row, so the keys of a row are
// unique and the K smallest of them are one set in one order, whatever the order in which the row's entries are met.
// A candidate that is not reported (-1), lies above the level, or is the row itself has the key kNoKey = ~0, which sorts
// behind every real key.
//
// The wave of neighbors.hip keeps the 64 smallest keys it has seen, ascending by lane, and reads the row 64 candidates
// at a time.  A chunk is sorted across the lanes by the bitonic network below (21 compare-exchange stages), then merged:
// lane l takes the smaller of its kept key and the sorted chunk's key of lane 63 - l -- the 64 smallest of the 128, as a
// bitonic sequence -- and six merge stages put them in ascending order.  The schedule of both is stated here as pure
// functions of (stage, lane); the kernel and tests/neighbors_host.cpp, which runs the same schedule over arrays of 64,
// both take it from here.
#pragma once
#include <stdint.h>

// (constexpr: the kernel takes the distances of the stages as template arguments)
#if defined(__HIPCC__)
#define NB_FN __host__ __device__ constexpr
#else
#define NB_FN constexpr
#endif

namespace edlib_amd {
namespace neighbors {

typedef unsigned long long u64;

constexpr int kLanes = 64;                      // candidates of a chunk, keys kept: one per lane
constexpr int kMaxK = 64;
constexpr int kRowsPerBlock = 4;                // waves of a block, a row each
constexpr int kSortStages = 21;                 // 1 + 2 + ... + 6
constexpr int kMergeStages = 6;
constexpr u64 kNoKey = ~0ull;

// ---- the key and the filter

// Is a candidate of reported distance d within `level` (level < 0: every reported distance)?
NB_FN bool within(int d, int level) { return d >= 0 && (level < 0 || d <= level); }

NB_FN u64 make_key(int d, int index) { return ((u64)(uint32_t)d << 32) | (uint32_t)index; }
NB_FN u64 candidate_key(int d, int index, int level) { return within(d, level) ? make_key(d, index) : kNoKey; }
NB_FN int key_distance(u64 key) { return (int)(key >> 32); }
NB_FN int key_index(u64 key) { return (int)(uint32_t)key; }

// ---- where the candidates of a row lie

// (1) a contiguous run of distances with an implicit index: candidate q of row t of a matrix of rowLength columns
NB_FN long long matrix_at(int rowLength, int t, int q) { return (long long)t * rowLength + q; }

// (2) the condensed vector of n sequences: pair (i, j), i != j, in either order.  For j > i the cells of row i are one
// contiguous stretch; for j < i it is one cell of each row above
NB_FN long long condensed_at(int n, int i, int j)
{
    const long long lo = i < j ? i : j, hi = i < j ? j : i;
    return (long long)n * lo - lo * (lo + 1) / 2 + (hi - lo - 1);
}

// (3) a CSR segment: candidate c of a row whose entries begin at `begin` (the partner and distance planes are read there)
NB_FN long long csr_at(long long begin, long long c) { return begin + c; }

// chunks of 64 a row of `length` candidates is read in
NB_FN long long chunks_of(long long length) { return (length + kLanes - 1) / kLanes; }

// ---- the schedule of the network

// Sort stage s = 0 .. 20: the phases p = 1 .. 6 make sorted runs of 2^p lanes, ascending where bit 2^p of the lane is
// clear and descending where it is set (so that two neighbouring runs are one bitonic sequence for the next phase; the
// last phase has one run, ascending); inside a phase the distances go 2^(p-1), ..., 2, 1.
NB_FN int sort_phase(int s)
{
    int p = 1;
    while (s >= p * (p + 1) / 2) ++p;
    return p;
}
NB_FN int sort_run(int s) { return 1 << sort_phase(s); }
NB_FN int sort_distance(int s)
{
    const int p = sort_phase(s);
    return 1 << (p - 1 - (s - p * (p - 1) / 2));
}
// Merge stage s = 0 .. 5 of a bitonic sequence of 64 into ascending order: distances 32, 16, ..., 1
NB_FN int merge_distance(int s) { return 32 >> s; }

// the lane a lane exchanges with at a distance
NB_FN int partner_lane(int lane, int distance) { return lane ^ distance; }
// does the lane keep the smaller of the two keys (else the larger)?  The lower lane of a pair keeps the smaller one in
// an ascending run, the larger one in a descending run
NB_FN bool sort_keeps_min(int s, int lane)
{
    const bool ascending = (lane & sort_run(s)) == 0;              // (the last phase's run is all 64 lanes)
    const bool lower = (lane & sort_distance(s)) == 0;
    return lower == ascending;
}
NB_FN bool merge_keeps_min(int s, int lane) { return (lane & merge_distance(s)) == 0; }

// the chunk's lane a lane meets in front of the merge
NB_FN int reversed_lane(int lane) { return kLanes - 1 - lane; }

// Does the lane take its partner's (key, payload)?  Equal keys are two kNoKey: neither side moves
NB_FN bool takes_partner(bool keepsMin, u64 mine, u64 other) { return keepsMin ? other < mine : other > mine; }

// what a row reports: the kept keys among the first K lanes
NB_FN int reported(int K, int kept) { return kept < K ? kept : K; }

}  // namespace neighbors
}  // namespace edlib_amd
