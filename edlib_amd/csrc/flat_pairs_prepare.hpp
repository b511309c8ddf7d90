// flat_pairs_prepare.hpp -- a flat pair set prepared on the device (DESIGN.md §4b "Streamed pairs"): the one definition
// of a flat descriptor, shared by the kernel that writes the descriptors of every pair and by the host's overflow rescan,
// and the launch interface of flat_pairs_prepare.hip.
#pragma once
#include "pair_kernels.hpp"

namespace edlib_amd {

constexpr int kFlatPosCap = 16;                   // end locations a flat unit's list keeps (more: the exact second pass)
constexpr int kFlatMaxQuery = 1024, kFlatMaxTarget = 65536;   // the flat envelope: 16 blocks, 65,536 columns

// What a flat descriptor depends on besides the pair's own offsets: the config and the reductions over the set
struct FlatShape {
    int scanMode;            // EDLIB_MODE_NW / SHW / HW as the kernels number them (0 / 1 / 2)
    int k;                   // config.k
    int ring;                // lanes of the phase-1 ring (4, 8, 16)
    int g32;                 // lanes of the rings of 32-row words
    int nwStore, ring32;     // NW PATH (the phase-1 scan is the storing scan); storing scans on rings of 32-row words
};

// columns of the target a unit's alignment can touch: the whole target (NW), at most 2 m + 1 (SHW: the scan stops there;
// HW: m + distance)
__host__ __device__ inline int flat_window(int scanMode, int m, int T)
{
    const long long w = 2LL * m + 1;
    return scanMode == 0 ? T : (int)(T < w ? T : w);
}

// rings of 32-row words take the storing scans whenever the set allows it: a store the kernel's 32-bit offsets reach (an NW
// store is cut into chunks instead), a Peq table per unit that fits a wave's LDS
__host__ __device__ inline bool flat_uses_ring32(bool paths, bool nwStore, long long store32Bytes, int g32, int sigmaT, int maxWords)
{
    return paths && (nwStore || store32Bytes < 0xF0000000LL) && ring32_lds_bytes(g32, sigmaT, maxWords) <= 48 * 1024;
}

// The phase-1 descriptor of pair u: query [qoff, qoff + m), target [toff, toff + T), its Peq at peqOff.  storeOff is the
// caller's (the store bases are a scan over the set).
__host__ __device__ inline PairDesc flat_desc(const FlatShape& s, int u, long long qoff, int m, long long toff, int T, long long peqOff)
{
    if (s.scanMode == 1) T = flat_window(1, m, T);               // (SHW: nothing beyond column 2m can tie the best)
    const int whole = m > T ? m : T;
    PairDesc x{};
    x.qoff = qoff; x.toff = toff; x.qlen = m; x.tlen = T; x.qstep = 1; x.tstep = 1;
    // NW: the ring holds every block of the unit, so the band is the whole matrix (threshold max(m, T)); SHW / HW:
    // columns scoring <= min(k, m) are end-location candidates
    x.kinit = s.scanMode == 0 ? whole : ((s.k < 0 || s.k > m) ? m : s.k);
    // NW with the column store: the first level of solveGlobalDistances -- the ring's band limit for a unit of more blocks
    // than the ring has lanes, capped by the caller's k; a unit that fails it sends the run to the general path
    if (s.nwStore) {
        const int kcap = s.k >= 0 ? s.k : 0x3fffffff;
        // (words of 32 rows on 8-lane rings, ring32_kernels.hip: a query of up to 8 words sits whole on its ring; above, the
        // first band level K = 128 -- well inside what the 4-lane rings of 64-row blocks hold, and inside ring32_max_k(8) = 192)
        const int level = s.ring32 ? ((m + 31) / 32 <= s.g32 ? whole : 128) : ((m + 63) / 64 <= s.ring ? whole : ring_max_k(s.ring));
        x.kinit = kcap < level ? kcap : level;
    }
    x.peqOff = peqOff;
    x.storeOff = 0; x.auxOff = 0; x.posCap = s.scanMode == 0 ? 0 : kFlatPosCap; x.posOff = (long long)u * kFlatPosCap;
    x.colOff = -1; x.bandT = 0; x.skip = 0; x.ring = s.ring;
    return x;
}

struct FlatPrepareArgs {
    int n;
    FlatShape shape;             // ring32 is decided on the device (the census gives sigmaT); the rest is the host's
    int paths, starts;           // op slots and store bases are wanted; reversed-query descriptors are wanted
    int maxWords;                // of the longest query, for the ring32 LDS test
    long long store32Bytes;      // sum of the ring32 stores (the same test)
    const uint8_t* tpool; long long tbytes;       // census: null = presence is already there (Create: the host's tables)
    const long long* qoff; const long long* toff; // [n + 1], rebased
    int sharedTarget;            // toff has two entries: every unit's target is [toff[0], toff[1])
    uint32_t* presence;          // [8]
    const int* cuts; int ncuts;  // ring32 NW store: first units of its chunks, then n (store bases are relative to the chunk)
    long long* sizes;            // scratch: [3][n + 1]
    long long* peqOff;           // [n + 1] scan of blocks x sigmaT
    long long* opsOff;           // [n + 1] scan of m + window + 8        (paths)
    long long* storeCum;         // [n + 1] scan of the store entries     (paths)
    long long* storeBase;        // [n]                                   (paths)
    PairDesc* descs;             // [n]
    PairDesc* revDescs;          // [n] (starts)
    int* iota;                   // [n] 0, 1, ...: the units whose alphabetLength is counted (may be null)
    unsigned long long* steps;   // [2] word-steps of a run: on the ring of 64-row blocks, on the rings of 32-row words
    void* tmp; size_t tmpBytes;  // rocPRIM scan scratch (flat_prepare_tmp_bytes)
};
hipError_t flat_prepare_tmp_bytes(int n, size_t* bytes);
// everything on `stream`, nothing waited for
hipError_t launch_flat_prepare(const FlatPrepareArgs& a, hipStream_t stream);

}  // namespace edlib_amd
