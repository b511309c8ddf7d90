// reads_kernels.hpp -- launch interface of the "reads-per-lane" scan family
// (many short queries against one shared target; BASELINE.json configs 2/3).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hit_list.hpp"
#include "segment_plan.hpp"

namespace edlib_amd {

constexpr int kMaxReadWords = 8;      // queries up to 256 symbols: one kernel instance per word count, every mode
// HW, banded kernel only: queries of 257..320 / ..384 / ..448 / ..512 symbols run in groups of 10 / 12 / 14 / 16 words (targets
// of up to 8 symbols), 513..768 / 769..1024 in groups of 24 / 32 words (four symbols); the row m-1 of a lane may sit in any of
// the group's last four (eight) words
constexpr int kMaxLongReadWords = 16;       // targets of 5..8 symbols
constexpr int kMaxLongReadWords4 = 32;      // targets of up to 4 symbols
constexpr int kFilterFromWords = 13;        // HW queries of this many words and more take the piece filter (long_reads.hip)
inline int read_group_words(int m) { const int w = (m + 31) / 32; return w <= kMaxReadWords ? w : (w <= 10 ? 10 : (w <= 12 ? 12 : (w <= 14 ? 14 : (w <= 16 ? 16 : (w <= 24 ? 24 : 32))))); }
// HW rows built bottom-aligned may carry R all-match rows above row m-1 (reads_kernels.hip: the score of the plain full-height
// scan then moves once per R + 1 columns): a group whose longest read leaves them room in its last word is eligible.  Seven
// rows (a byte per group of eight columns) where they fit, else three (a nibble per four), else none.
constexpr int kDelayRowsDeep = 7, kDelayRowsShallow = 3;
constexpr bool delay_rows_fit(int nwords, int longest, int rows) { return nwords <= kMaxReadWords && longest >= 1 && longest + rows <= 32 * nwords; }
constexpr int delay_rows_for(int nwords, int longest)
{
    return delay_rows_fit(nwords, longest, kDelayRowsDeep) ? kDelayRowsDeep : (delay_rows_fit(nwords, longest, kDelayRowsShallow) ? kDelayRowsShallow : 0);
}
// bottomAlign values of the Peq builder and ReadScanArgs::bottomAligned: 0 top-aligned, 1 bottom-aligned, 1 + R with R delay rows
constexpr bool bottom_align_valid(int b) { return b == 0 || b == 1 || b == 1 + kDelayRowsShallow || b == 1 + kDelayRowsDeep; }
constexpr int kLanes = 64;            // wave64, hard-coded (gfx950)

// Hit-list read batches (reads_hits.hip): the HITS scans append closed runs of columns scoring <= k to the
// device list (hit_list.hpp) with the key (slotBase + slot) << 32 | firstEnd and four planes: lastEnd, editDistance,
// endLocation, numLocations of the run.

// Everything the scan kernel needs; plain pointers into HBM.
struct ReadScanArgs {
    const uint32_t* peq;      // [readBlock][S symbols][NWD words][64 lanes], S = 4 (both kernels), 8 or 16 (banded kernel)
    const uint32_t* tpk;      // target, 2 bits / symbol, 16 symbols / dword, LSB first (scan_reads_kernel)
    const uint32_t* trows;    // target, 16 bits / symbol = LDS row offset (symbol << 8), 16 columns per 32-byte block,
                              // padded by two blocks (scan_reads_banded_kernel)
    int targetLength;
    const int* qlen;          // [slots] query length of the read in that slot (>= 1)
    const int* kinit;         // [slots] initial threshold: columns scoring <= kinit are candidates
    const int* slotmap;       // optional [lanes] lane -> slot indirection (second, exact pass)
    int nlanes;               // number of lanes to run (slots, or entries of slotmap)
    int numSegments;          // target split into this many segments (HW only; else 1)
    int segLen;               // columns per segment, multiple of 16
    int warm;                 // warm-up columns before a segment (2*maxQueryLen-1 for HW)
    int* segBest;             // [lanes][numSegments] best score seen in the segment (NW: final score)
    int* segCnt;              // [lanes][numSegments] number of columns attaining it
    int* segPos;              // positions pool
    int cap;                  // positions kept per (lane, segment) when posOff == nullptr
    const long long* posOff;  // optional [lanes][numSegments] offset into segPos (exact pass)
    const int* posCap;        // optional [lanes][numSegments] capacity (exact pass)
    int kcap;                 // banded HW kernel: effective threshold = min(kinit[slot], kcap)
    unsigned long long* wordSteps;   // banded HW kernel: += 32-row word-columns actually computed (may be null)
    // scan_reads_full_kernel, strips of a taller query (null: a whole query per lane).  One dword per 16 columns and lane, two
    // bits per column (bit 0: +1, bit 1: -1): the horizontal deltas of the bottom row of the strip above (in) / of this strip
    // (out), laid out [segment][block of 16 columns][lane of the producing launch]
    const uint32_t* chainIn; uint32_t* chainOut;
    const int* chainSrc;      // [lanes] lane of the producing launch that holds the strip above
    int chainInLanes;         // nlanes of the producing launch
    int chainBlocks;          // blocks of 16 columns per segment in the streams (>= (segLen + warm) / 16 + 2)
    const int* rowBase;       // [slots] query rows above the strip (its bottom row starts at score rowBase + qlen); null: 0
    int filter;               // banded HW kernel: 1 = fixed threshold, segPos lists the 16-column BLOCKS that hold a column
                              // scoring <= kinit (each once), segCnt their number (piece filter of long reads)
    HitList hits;             // HITS instantiation of the banded kernel only (launch_scan_reads_hits)
    int slotBase;             // ... the launch's group starts at this slot of the batch-wide slot table
    int bottomAligned;        // scan_reads_kernel, HW only: peq was built with this bottomAlign (1: row m-1 at bit 31 of the last
                              // word; 1 + R: at bit 31 - R under R = 3 or 7 delay rows)
    int* liveBest;            // scan_reads_kernel on bottom-aligned rows: optional [lanes] running best of the lane over ALL its
                              // segments, set to the lane's threshold before the launch (no slotmap).  The segments start
                              // from it, publish what they find and pick it up again every kLivePeriod columns.  Null: every
                              // (lane, segment) keeps a best of its own, from kinit
    const Segment* segTable;  // scan_reads_kernel only: optional [numSegments] columns of every segment, ascending, starts
                              // multiples of 16 (plan_segments_tapered).  Null: segment s is [s segLen, (s + 1) segLen)
#ifdef EDLIB_AMD_DRAIN_DIAG
    unsigned long long* waveClock;   // diagnostic build: optional [2][waves of the launch] s_memrealtime at entry / exit
#endif
};
constexpr int kLivePeriod = 1024;     // columns between two looks at liveBest (a multiple of 16)

// mode: 0 NW, 1 SHW, 2 HW (values of EdlibAlignMode).  Returns hipSuccess or the launch error.
hipError_t launch_scan_reads(int nwords, int mode, const ReadScanArgs& a, hipStream_t stream);
// workgroups of the bottom-aligned HW scan_reads_kernel that the current device holds at once (occupancy x CUs)
hipError_t scan_reads_resident_workgroups(int nwords, int bottomAligned, int* resident);

// HW only: Ukkonen-banded variant with k-doubling (see reads_kernels.hip); same Peq layout.  syms = Peq rows per word:
// 4, 8 or 16 (target symbols rounded up); launch_scan_reads only knows 4.
hipError_t launch_scan_reads_banded(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream);

// HW only, no band: every row of every column with the banded kernel's data path (syms = 4, 8 or 16)
hipError_t launch_scan_reads_full(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream);

hipError_t launch_pack_target_2bit(const uint8_t* raw, const uint8_t* lut, int targetLength,
                                   uint32_t* tpk, hipStream_t stream);
// ndwords = 8 * (blocks of 16 columns, including the two blocks of padding): every dword is written
hipError_t launch_pack_target_rows(const uint8_t* raw, const uint8_t* lut, int targetLength,
                                   uint32_t* trows, int ndwords, hipStream_t stream);

// Builds Peq for every slot (reference buildPeq, edlib.cpp:358-384, for the <= syms target symbols; eqtbl[byte] =
// 16-bit set of the target symbols a query byte equals),
// the per-slot query length and the number of query byte values absent from the target.
// bottomAlign 1: query row i at bit 32 nwords - m + i and the bits below set in every row (ReadScanArgs::bottomAligned);
// 1 + R (R = 3 or 7 delay rows): at bit 32 nwords - R - m + i, the R bits above row m-1 set in every row as well.
hipError_t launch_build_peq_reads(int nwords, int syms, const uint8_t* reads, const long long* qoff,
                                  const int* perm, int nslots, const uint16_t* eqtbl,
                                  const uint32_t* targetPresence /*8 dwords*/, int kcfg,
                                  uint32_t* peq, int* qlen, int* kinit, int* alphaExtra,
                                  hipStream_t stream, int bottomAlign = 0);

// Piece filter: gathers the (lane, block) candidates of a filter scan into one list.  out[2i] = lane, out[2i+1] = block;
// *counter = number of candidates (may exceed maxOut: the caller retries with a larger list); overflow[lane] = 1 when a
// (lane, segment) record held more than `cap` blocks.
hipError_t launch_collect_candidates(const int* segCnt, const int* segPos, int numSegments, int cap, int nlanes,
                                     int* out, int maxOut, int* counter, int* overflow, hipStream_t stream);

// Exact k-mer seed filter, the first pass of HW groups of up to kMaxReadWords words against a target of at most four
// symbols (reads_seed.hip).  Buckets on the first kSeedQ symbols of every target position.
constexpr int kSeedQ = 12;
constexpr int kSeedBuckets = 1 << (2 * kSeedQ);
constexpr int kSeedBucketCap = 64;      // a piece whose bucket holds more target positions hands its read back
constexpr int kSeedMaxDiag = 32;        // distinct diagonals a read may collect (LDS: 8 KB per wave)
constexpr int kSeedMaxWindow = 1024;    // columns of one merged window

struct SeedArgs {
    const uint32_t* peq;      // the group's Peq rows, [readBlock][4][NWD][64 lanes]
    const int* qlen;          // [slots]
    const int* perm;          // [slots] slot -> unit, -1 = padding
    const uint32_t* tpk;      // target, 2 bits / symbol (ReadScanArgs::tpk)
    int targetLength;
    const uint32_t* seedOff;  // [kSeedBuckets + 1]
    const uint32_t* seedPos;  // [targetLength]
    int nslots;               // multiple of 64
    int k;                    // threshold: columns scoring <= k are found
    int* best; int* total; int* pos; int* flags;   // the group's merged per-slot results (merge_segments_kernel's meaning)
    int* backSlots; int* backCount;                // slots handed back to the banded scan
    unsigned long long* wordSteps;                 // += word-columns verified
    HitList hits;                                  // HITS variant only (launch_seed_verify_hits): runs instead of best / total / pos / flags
    int slotBase;                                  // ... the group's first slot in the batch-wide slot table
};

hipError_t seed_index_scratch_bytes(size_t* bytes);
// cnt, off: kSeedBuckets + 1 entries; pos: targetLength entries; tmp: seed_index_scratch_bytes()
hipError_t launch_build_seed_index(const uint32_t* tpk, int targetLength, uint32_t* cnt, uint32_t* off, uint32_t* pos,
                                   void* tmp, size_t tmpBytes, hipStream_t stream);
hipError_t launch_seed_verify(int nwords, const SeedArgs& a, hipStream_t stream);

hipError_t launch_merge_segments(const int* segBest, const int* segCnt, const int* segPos,
                                 int numSegments, int cap, int nlanes, const int* slotmap, int capFinal,
                                 int* best, int* total, int* pos, int* flags, hipStream_t stream, int gatherFlag = 1);
// flags[] of the merge: the slot's list is scanned again / is complete in the records of the last level / of the group's pass 1
constexpr int kOvfRescan = 1, kOvfGatherLevel = 2, kOvfGatherGroup = 4;
// exact pass without a scan for n slots whose contributing segments all fit `cap`: the complete ascending list of entry e
// (records of scan lane idx[e]) goes to out + off[e], at most lim[e] positions
hipError_t launch_gather_segments(const int* segBest, const int* segCnt, const int* segPos, int numSegments, int cap, int n,
                                  const int* idx, const long long* off, const int* lim, int* out, hipStream_t stream);

// Ascending lists of a group's slots, compacted on the device (rocPRIM select; tmp: select_slots_scratch_bytes(nslots)).
// Open slots: real (perm >= 0), nothing found (total <= 0) and a threshold min(qlen, k; kcfg < 0: qlen) above kDone.
// Flagged slots: real and flags != 0.  *count (device) = length of the list.
// Both-strand groups (strands.hpp, mates in the slots s and s ^ 1): `mates` closes a slot whose mate has found something,
// `win` (the pairs' codes) drops the flagged slots whose mate is the one reported.
hipError_t select_slots_scratch_bytes(int nslots, size_t* bytes);
hipError_t launch_select_open_slots(const int* perm, const int* total, const int* qlen, int kcfg, int kDone, int nslots,
                                    int* out, int* count, void* tmp, size_t tmpBytes, hipStream_t stream, bool mates = false);
hipError_t launch_select_flagged_slots(const int* perm, const int* flags, int nslots, int* out, int* count,
                                       void* tmp, size_t tmpBytes, hipStream_t stream, const int* win = nullptr);
// out[3 i ..] = {slots[i], flags[slots[i]], total[slots[i]]}
hipError_t launch_pick_slot_records(const int* slots, int n, const int* flags, const int* total, int* out, hipStream_t stream);

// ---- hit-list read batches (reads_hits.hip): every maximal run of columns scoring <= k, HW, up to
// kMaxReadWords words.  The HITS instantiations keep the threshold at kinit[slot] for the whole scan and append each closed
// run to a.hits; segBest / segCnt / segPos are not touched (cap = 1, the rest null).
hipError_t launch_scan_reads_hits(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream);
// seed_verify_kernel at threshold a.k with runs instead of the best-16 record; same hand-back list
hipError_t launch_seed_verify_hits(int nwords, const SeedArgs& a, hipStream_t stream);
// The finish of a Run over the settled list (hit_list.hpp).  slotUnit: batch-wide slot -> unit, -1 = padding.
//   keys become (unit << 32) | firstEnd and are sorted; runs of a unit that meet at a segment boundary (lastEnd + 1 == next
//   firstEnd) are stitched into hl.out() as firstEnd, lastEnd, editDistance, endLocation, numLocations, five int arrays of
//   *total entries each, and hl.off() [numUnits + 1] comes from the stitched list's units.
// hl.extra: kReadHitsExtraBytes per entry (head, at: dwords; outUnit: ints); total: one long long
constexpr int kReadHitsExtraBytes = 12;
hipError_t launch_read_hits_finish(HitListBuffers& hl, const int* slotUnit, int numUnits, long long* total, hipStream_t stream);

}  // namespace edlib_amd
