// pairs_gather.hpp -- launch interface of the gather that fills the pools of a flat pair set from a window batch
// (edlibAmdBatchPairsSetWindows; pairs_gather_core.hpp: what a thread does).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edlib_amd {

// What a window batch lends to the gather: device pointers that stay valid, and unwritten, while the window batch is not
// given new units or destroyed; and the host's copy of what the set is planned from.  A read batch (Batch::gatherSource)
// lends the same with its raw target in place of the pack; its pointers hold until it is destroyed.
struct WindowSource {
    int numQueries = 0, targetLength = 0;
    const long long* h_qoff = nullptr;            // host: [numQueries + 1] offsets of the queries as the caller gave them, from any base
    const uint8_t* d_qpool = nullptr; size_t qpoolBytes = 0;       // the query pool (both strands of every query where stranded)
    const long long* d_qoff = nullptr;            // offsets of its entries: entry q, or 2 q + strand where stranded
    bool stranded = false;
    const uint32_t* d_pack = nullptr; long long packDwords = 0;    // the target, 4-bit codes, 8 columns per dword from dword 0
    uint8_t idToByte[16] = {};                    // code -> byte
    // ... or, in place of the pack, the target as its bytes (a read batch: edlibAmdBatchPairsSetSharedWindows): 4-byte
    // aligned, tbytesAlloc bytes allocated (>= targetLength)
    const uint8_t* d_tbytes = nullptr; size_t tbytesAlloc = 0;
    const char* what = "the window batch";        // the source in a refusal
};

struct PairsGatherArgs {
    int numPairs;                                 // >= 1
    const long long* qoff; const long long* toff; // device: [numPairs + 1] offsets of the destination pools, from 0
    long long qbytes, tbytes;                     // qoff[numPairs], toff[numPairs]
    const int* pairQuery; const int* pairStart; const uint8_t* pairStrand;    // device; pairStrand null: all forward
    uint8_t* qpool; uint8_t* tpool;               // device: qbytes + 16 and tbytes + 16 bytes, 16-byte aligned
};

// Writes both pools with their 16 trailing zero bytes on `stream`.  Every tuple has been checked against the source by
// the caller: the kernel checks none.
hipError_t launch_pairs_gather(const WindowSource& src, const PairsGatherArgs& a, hipStream_t stream);

// What a cross or self batch lends to the gather (CrossBatch::gatherSource; edlibAmdBatchPairsSetCells): its query pool and
// the pack of its targets back to back, device pointers that stay valid, and unwritten, while the batch is not given new
// targets or destroyed; and the host's copy of what the checks need, linear in the counts.
struct CellSource {
    int numQueries = 0, numTargets = 0;
    const int* h_qlen = nullptr;                  // host: [numQueries] length of every query
    const int* h_tlen = nullptr;                  // host: [numTargets] length of every target
    const uint8_t* h_inPack = nullptr;            // host: [numTargets] 1 where the target is in the pack (null: none is)
    const uint8_t* d_qpool = nullptr; size_t qpoolBytes = 0;       // the query pool (both strands of every query where stranded)
    const long long* d_qoff = nullptr;            // offsets of its entries: entry q, or 2 q + strand where stranded
    bool stranded = false;
    const uint32_t* d_pack = nullptr; long long packDwords = 0;    // 4-bit codes, every target from a dword of its own
    const long long* d_tdw = nullptr;             // [targets in the pack] first dword of the target at each place of the pack's order
    const int* d_place = nullptr;                 // [numTargets] place of every target in that order (-1: not in the pack)
    uint8_t idToByte[16] = {};                    // code -> byte
    const char* what = "the cross batch";         // the source in a refusal
    bool self = false;                            // one set: a query index and a target index name sequences of it
};

// place[tperm[i]] = i for the `numSorted` targets of a pack in its order (place: numTargets ints, the others become -1)
hipError_t launch_pack_places(const int* tperm, int numSorted, int* place, int numTargets, hipStream_t stream);

struct CellsGatherArgs {
    PairsGatherArgs pools;                        // pairStart: device, or null where every pair takes its whole target
    const int* pairTarget;                        // device
    long long* pairBase;                          // device scratch: [numPairs]
};

// The same pools from a cross batch's pack: the plan kernel writes every pair's 64-bit nibble base, the target gather
// reads the pack from there, the query gather is launch_pairs_gather's.  Every tuple has been checked by the caller.
hipError_t launch_pairs_gather_cells(const CellSource& src, const CellsGatherArgs& a, hipStream_t stream);

}  // namespace edlib_amd
