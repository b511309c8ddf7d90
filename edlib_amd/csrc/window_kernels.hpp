// window_kernels.hpp -- launch interface of the window kernels (units = a query against a window of one resident target,
// DISTANCE only): the lane-per-unit scan and the best unit per query.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edlib_amd {

// What the scan of one word group needs.  Lane l of wave w takes sorted unit 64 w + l of the group.
struct WindowScanArgs {
    const uint32_t* peq;        // the group's Peq, [slot / 64][S][NWD][slot % 64] (build_peq_reads_kernel)
    const int* qlen;            // [slots]
    const uint32_t* tpk;        // the target, 4 bits per column, 8 columns per dword, column 0 in bits 0..3 of dword 0
    int targetLength;           // columns of tpk: no window reaches past it (checked at Create)
    const int* uslot;           // [numSorted] query slot of the sorted unit
    const int* ustart;          // [numSorted] first target column of its window
    const int* ulen;            // [numSorted] columns of its window, ascending within the group
    const int* uperm;           // [numSorted] sorted unit -> unit index
    int numSorted;
    int kcfg;
    int* ed; int* nloc; int* end;   // [numUnits]
};

// nwords 1..8, syms 4 / 8 / 16, mode 0 NW / 1 SHW / 2 HW
hipError_t launch_scan_windows(int nwords, int syms, int mode, const WindowScanArgs& a, hipStream_t stream);

// Per query over the units that name it: best unit / best distance / second distance into best [3][numQueries], through
// bkey [2][numQueries] (the order-free atomicMin scheme of cross_hits.hip over keys (distance << 32) | unit).
hipError_t launch_window_best(const int* unitQuery, const int* ed, int numUnits, int numQueries,
                              unsigned long long* bkey, int* best, hipStream_t stream);

// ---- the queries and the unit list prepared on the device (window_units.hip)
constexpr int kWindowNoGroup = 8;               // key of a pool entry no unit names: behind the word groups 1..8

// qoff of the query pool from the caller's offsets offIn [numQueries + 1] (any base): rebased, [numQueries + 1]; stranded:
// of the pool of both strands, [2 numQueries + 1], entry 2 q the query and 2 q + 1 its reverse complement
hipError_t launch_window_query_offsets(const long long* offIn, int numQueries, bool stranded, long long* qoff,
                                       hipStream_t stream);

// What the preparation of a unit list reads and writes.  Entry of unit u: unitQuery[u], or 2 unitQuery[u] + unitStrand[u]
// where unitStrand is not NULL (numEntries = numQueries or twice that).  The host has checked every unit: the query in
// [0, numQueries), the strand 0 or 1, the query at most 256 bases, the length in [0, 65,536].
struct WindowUnitsArgs {
    const long long* offIn;                     // [numQueries + 1] the caller's query offsets
    const int* unitQuery; const int* unitStart; const int* unitLength;    // [numUnits] as the caller gave them
    const unsigned char* unitStrand;            // [numUnits] or NULL
    int numUnits, numEntries;
    // scratch
    unsigned char* named;                       // [numEntries] 1: a unit names the entry
    uint32_t* ukey; uint32_t* uval; uint32_t* ukeySorted;                 // [numUnits]
    uint32_t* ekey; uint32_t* eval; uint32_t* ekeySorted;                 // [numEntries]
    int* slotOf;                                // [numEntries] slot of a named entry in its word group
    // results
    int* entSorted;                             // [numEntries] the named entries by (word group, entry), the others behind
    int* bound;                                 // [kWindowNoGroup + 1] entries of word group w: [bound[w - 1], bound[w])
    int* uslot; int* ustart; int* ulen; int* uperm;   // [numUnits] by (word group, window length, unit): the scan's arrays
};
// temporary bytes of launch_window_units_prepare
hipError_t window_units_tmp_bytes(int numUnits, int numEntries, size_t* bytes);
// Everything above on `stream`; nothing where numUnits is 0.  Units of word group w are the sorted positions behind those
// of the groups below it (the host has counted them); the group's slots are entSorted[bound[w - 1] .. bound[w]).
hipError_t launch_window_units_prepare(const WindowUnitsArgs& a, void* tmp, size_t tmpBytes, hipStream_t stream);

}  // namespace edlib_amd
