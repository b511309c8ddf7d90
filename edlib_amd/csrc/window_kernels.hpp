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

}  // namespace edlib_amd
