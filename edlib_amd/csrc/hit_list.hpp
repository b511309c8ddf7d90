// hit_list.hpp -- the one device hit list of the batches whose result is a list of unknown length: hit-list read batches
// (DESIGN.md §3e), hit-list cross and self batches and occurrence cross batches (§4h).  A scan appends (64-bit key, P ints)
// entries through one counter (HitList, hit_list_append); the host side (HitListBuffers, hit_list.hip) owns the buffers,
// grows them to the count of a Run that overflowed them, takes the rows answered off the kernel, sorts (key, index) with
// rocPRIM's radix sort, and makes the CSR form -- offsets per row, the planes gathered in sorted order -- that crosses the
// link as one pinned block.
//
// Where the host's rows sit in the unsorted list does not matter (they go behind the device's), in any of the four kinds:
//   * read keys (unit, firstEnd) are unique: a column closes one run of a unit;
//   * cross and self keys are unique per cell, and a cell is answered by one engine;
//   * an occurrence cell's runs share a key, but they all come from one producer (the kernel's lane, or one internal
//     session) in ascending column order, and the radix sort is stable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace edlib_amd {

// What a scan needs of the list.  count may pass cap: nothing is written at or past it, and the host grows the list to
// the count and scans again.
struct HitList {
    unsigned long long* count;  // entries appended so far
    unsigned long long* key;    // [cap]
    int* val;                   // [P][cap]
    unsigned long long cap;
};

// Appends (key(), v) of every lane with `emit`: one 64-bit atomic per wave among the lanes that are active at the call
// (ballot, mbcnt rank, the first emitting lane adds, readlane of the base), so it holds inside divergent code.  key: a
// callable, called only for an entry that is written -- the caller's key stays out of the registers that are live across
// the atomic (a key made in front of the call cost the read HITS scans one or two VGPRs and two more spills).  Returns the
// entry's index: >= h.cap where it was counted but not written, ~0 for a lane without `emit`.
template <int P, typename Key>
__device__ __forceinline__ unsigned long long hit_list_append(const HitList& h, const bool emit, Key&& key, const int (&v)[P])
{
    typedef unsigned long long u64;
    const u64 bal = __builtin_amdgcn_ballot_w64(emit);
    if (!bal) return ~0ull;
    const int lead = __builtin_ctzll(bal);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    u64 base = 0;
    if (emit && rank == 0) base = atomicAdd(h.count, (u64)__popcll(bal));
    base = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(base >> 32), lead) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)base, lead);
    const u64 at = base + rank;
    if (emit && at < h.cap) {
        h.key[at] = key();
#pragma unroll
        for (int f = 0; f < P; ++f) h.val[f * h.cap + at] = v[f];
    }
    return emit ? at : ~0ull;
}

// Rows answered on the host (empty reads, the cells of the internal sessions): keys, the planes, and the byte of each
// where the list carries one
struct HitRows {
    std::vector<unsigned long long> key;
    std::vector<int> val[5];
    std::vector<uint8_t> byte;
    size_t size() const { return key.size(); }
    void clear() { key.clear(); byte.clear(); for (auto& v : val) v.clear(); }
};

// The buffers of one list and the steps every kind of batch takes with them.  A Run: reset(), the owner's scans, settle()
// (the count, growth and a second scan, the host's rows), the owner's own key rewrite if any, sort(), then offsets() and
// gather() or the owner's own finish over skey / sidx into off() / out(); a view: fetch().
struct HitListBuffers {
    // prefix and noun of the error texts ("cross batch", "hits"); planes: P; limitBits: a list holds 2^limitBits - 1
    // entries (31 where the owner's finish indexes with int, else 32: the sort's index); bytePlane: a byte per entry
    // (strands); extraBytes: per-entry bytes of the owner's own in `extra`
    void configure(const char* prefix, const char* noun, int planes, int limitBits, bool bytePlane, int extraBytes) {
        prefix_ = prefix; noun_ = noun; planes_ = planes; limitBits_ = limitBits; bytePlane_ = bytePlane; extraBytes_ = extraBytes;
    }
    // The counter, the pinned count, room for off [rows + 1]; the list for at least minCap entries (a larger one is kept)
    int size(size_t rows, long long minCap, hipStream_t stream);
    HitList list() const { return HitList{count.p, key.p, val.p, (unsigned long long)cap}; }
    hipError_t reset(hipStream_t stream) { return hipMemsetAsync(count.p, 0, sizeof(unsigned long long), stream); }   // before the scans
    // After the scans: reads the count; where count + rows exceeds the capacity the list grows to that and rescan() (the
    // owner's scans, enqueued again) runs once behind a reset -- later Runs fit --, a second overflow is an error; then
    // the rows behind the device's entries.  n is the sum.
    template <typename Scan>
    int settle(const HitRows& rows, hipStream_t stream, Scan&& rescan) {
        for (int attempt = 0; ; ++attempt) {
            const int s = afterScan(rows, attempt, stream);
            if (s != kScanAgain) return s;
            if (rescan()) return 1;
        }
    }
    // (key, idx) -> (skey, sidx) over the low 32 bits and as many high bits as highValues - 1 needs; n = 0: nothing
    hipError_t sort(long long highValues, hipStream_t stream);
    hipError_t needScratch(size_t bytes) { return tmp.ensure(bytes); }     // before the finish is enqueued
    // off[r] = first sorted entry whose high half is r or more, for the rows size() was given (r = rows: n)
    hipError_t offsets(hipStream_t stream);
    // out [P + 1][n]: the low half of the sorted key, then the planes by sidx; byteOut [n] likewise.  outN = n
    hipError_t gather(hipStream_t stream);
    // off [rows + 1] then `planes` x outN ints of out -- they lie back to back on the device -- as one pinned block, in one
    // copy, once per Run
    int fetch(int planes, hipStream_t stream, const long long** off, const int** out);

    long long cap = 0, n = 0, outN = 0;                         // capacity; entries of the filled list, of the finished one
    DevBuf<unsigned long long> count, key, skey;
    DevBuf<int> val;                                            // [P][cap] as appended
    DevBuf<uint32_t> idx, sidx;                                 // idx: iota, written when the list grows
    DevBuf<uint8_t> byte, byteOut, extra, tmp;                  // tmp: the sort's scratch, and the owner's finish's
    DevBuf<uint8_t> res;                                        // the finished list: off [rows + 1], then out [P + 1][outN]
    long long* off() const { return reinterpret_cast<long long*>(res.p); }
    int* out() const { return reinterpret_cast<int*>(res.p + (rows_ + 1) * sizeof(long long)); }
    PinBuf pinned;                                              // the count, then a word of the owner's
    unsigned long long* pinnedWord() const { return reinterpret_cast<unsigned long long*>(pinned.p) + 1; }
    PinnedPart result;

private:
    int grow(long long cap, hipStream_t stream);
    hipError_t allocResult(size_t c) { return res.alloc((rowsCap_ + 1) * sizeof(long long) + ((size_t)planes_ + 1) * c * sizeof(int)); }
    static constexpr int kScanAgain = 2;
    int afterScan(const HitRows& rows, int attempt, hipStream_t stream);     // 0 settled, 1 error, kScanAgain
    const char* prefix_ = ""; const char* noun_ = "";
    int planes_ = 0, limitBits_ = 32, extraBytes_ = 0;
    bool bytePlane_ = false;
    size_t rows_ = 0, rowsCap_ = 0;                             // rows of this Run's offsets; rows res has room for
};

}  // namespace edlib_amd
