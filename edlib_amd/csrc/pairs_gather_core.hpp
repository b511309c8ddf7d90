// pairs_gather_core.hpp -- the pools of a pair batch gathered from a window batch (edlibAmdBatchPairsSetWindows, DESIGN.md
// §4b "Pairs from a window batch"): what one THREAD does.
//
// The destination is a pool of a flat pair set: the sequences of the pairs back to back (off[p] .. off[p + 1] is pair p's)
// and 16 zero bytes behind them.  A thread owns one aligned run of kRun = 16 destination bytes and writes it with one
// store.  It finds the pair its first byte belongs to by a binary search of the offsets, then walks the pairs its run
// spans: a run that crosses a pair boundary is composed from both pairs in registers, so no two threads ever write into
// one dword and nothing is atomic.  Bytes behind the last pair are zero.
//
//   target pool: the source is the window batch's 4-bit pack (8 columns per dword, LSB first, from dword 0).  Eight codes
//     at any nibble position are the two dwords around it funnel-shifted by the nibble phase (codes8); a 256-entry table
//     of byte pairs (tab2[c] = idToByte[c & 15] | idToByte[c >> 4] << 8) expands two codes per lookup (expand8).
//   query pool: the source is the window batch's query pool.  Eight bytes at any byte position are the three dwords around
//     it funnel-shifted by the byte phase (bytes8).  Strand 1 of a pair reads the reverse-complement entry of a stranded
//     pool as it is; from a plain pool it reads the same bytes from the far end, byte-swapped and complemented through a
//     256-entry table (revcomp8).
//   target pool from a read batch (edlibAmdBatchPairsSetSharedWindows, "Pairs from a read batch"): the source is the raw
//     target.  Sixteen bytes at any byte position are five dwords funnel-shifted (bytes16); at a pair boundary, bytes8.
//   target pool from a cross or self batch (edlibAmdBatchPairsSetCells, "Pairs from a cross batch"): the source is the
//     batch's pack of many targets, each from a dword of its own; a pair's window starts at a 64-bit nibble position
//     (TargetCellsSource, target_run_cells), the rest is the window batch's codes8 / expand8.
//
// This header compiles for the device (pairs_gather.hip) AND for the host (tests/pairs_gather_host.cpp: the same code, the
// runs walked one by one, checked against numpy slicing: tests/test_pairs_gather_model.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FN __host__ __device__ __forceinline__
#else
#define PG_FN static inline __attribute__((always_inline))
#endif

namespace edlib_amd {
namespace pairs_gather {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr int kRun = 16;                          // destination bytes per thread: one 128-bit store
constexpr int kBlockThreads = 256;
constexpr int kBlockBytes = kRun * kBlockThreads; // destination bytes per block

struct Run { u64 w[2]; };                         // the 16 bytes of a run, byte i of the run = bits 8 i .. of w[i / 8]

// The source of the query pool: the window batch's pool as dwords (ndw of them), the offsets of its entries (entry q, or
// 2 q + strand where the pool is stranded), and per pair the query and the strand (null: all forward)
struct QuerySource {
    const u32* pool; long long ndw;
    const long long* off;
    int stranded;
    const int* pairQuery;
    const uint8_t* pairStrand;
};
// The source of the target pool: the pack as dwords (ndw of them) and per pair the first column of its window
struct TargetSource {
    const u32* pack; long long ndw;
    const int* pairStart;
};

// the largest p in [lo, hi] with off[p] <= pos (off[lo] <= pos)
PG_FN int find_pair(const long long* off, int lo, int hi, long long pos)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The same search by kProbes probes a step, for a wave whose lanes all look for one position: lane l reads the offset at
// probe_at(lo, hi, l); the probes whose offset is <= pos are a prefix (offsets ascend), and with their number narrow()
// leaves a range of at most (hi - lo) / kProbes + 1 pairs: three steps from 262,144 pairs instead of eighteen dependent
// loads.  A probe past hi is not read and counts as greater.
constexpr int kProbes = 64;
PG_FN int probe_step(int lo, int hi) { return (hi - lo) / kProbes + 1; }
PG_FN long long probe_at(int lo, int hi, int lane) { return (long long)lo + (long long)(lane + 1) * probe_step(lo, hi); }
PG_FN void narrow(int& lo, int& hi, int count)
{
    const int step = probe_step(lo, hi);
    lo += count * step;
    hi = lo + step - 1 < hi ? lo + step - 1 : hi;
}
// what the wave's ballot counts, lane by lane (the host's form of a step)
PG_FN int count_probes(const long long* off, int lo, int hi, long long pos)
{
    int count = 0;
    for (int lane = 0; lane < kProbes; ++lane) {
        const long long at = probe_at(lo, hi, lane);
        if (at <= hi && off[at] <= pos) ++count;
    }
    return count;
}

// The positions a block looks for: its first byte and its last (n >= 1 pairs, total = off[n] >= 1); the pairs [lo, hi]
// they lie in hold every byte of the block.  A pair has at least one byte, so the last byte lies at most kBlockBytes pairs
// behind the first: block_far() bounds the second search.
PG_FN long long block_first(long long total, long long block) { const long long b = block * kBlockBytes; return b < total - 1 ? b : total - 1; }
PG_FN long long block_last(long long total, long long block)
{
    const long long b = block * kBlockBytes + kBlockBytes - 1;
    return b < total - 1 ? b : total - 1;
}
PG_FN int block_far(int lo, int n) { return (long long)lo + kBlockBytes < n - 1 ? lo + kBlockBytes : n - 1; }

PG_FN u32 dword_at(const u32* p, long long ndw, long long i) { return i < ndw ? p[i] : 0u; }

// ({hi, lo} >> sh) & 0xffffffff, sh in 0..31
PG_FN u32 funnel(u32 lo, u32 hi, int sh) { return sh ? (lo >> sh) | (hi << (32 - sh)) : lo; }

// the eight 4-bit codes from nibble position s on, code j in bits 4 j ..
PG_FN u32 codes8(const u32* pack, long long ndw, long long s)
{
    const long long i = s >> 3;
    return funnel(dword_at(pack, ndw, i), dword_at(pack, ndw, i + 1), 4 * (int)(s & 7));
}

// eight codes to their eight bytes
PG_FN u64 expand8(u32 v, const uint16_t* tab2)
{
    return (u64)tab2[v & 255] | (u64)tab2[(v >> 8) & 255] << 16 | (u64)tab2[(v >> 16) & 255] << 32 | (u64)tab2[v >> 24] << 48;
}

// the eight bytes from byte position s on
PG_FN u64 bytes8(const u32* pool, long long ndw, long long s)
{
    const long long i = s >> 2;
    const int sh = 8 * (int)(s & 3);
    const u32 d0 = dword_at(pool, ndw, i), d1 = dword_at(pool, ndw, i + 1), d2 = dword_at(pool, ndw, i + 2);
    return (u64)funnel(d0, d1, sh) | (u64)funnel(d1, d2, sh) << 32;
}

// bytes 0 .. cnt - 1 of x in reverse order, each complemented (comp: the 256 complements of strands.hpp)
PG_FN u64 revcomp8(u64 x, int cnt, const uint8_t* comp)
{
    u64 r = 0;
    for (int j = 0; j < 8; ++j)
        if (j < cnt) r |= (u64)comp[(x >> (8 * (cnt - 1 - j))) & 255] << (8 * j);
    return r;
}

// bytes 0 .. cnt - 1 of e become the bytes at .. at + cnt - 1 of the run (1 <= cnt <= 8, at + cnt <= 16)
PG_FN void put(Run& r, int at, u64 e, int cnt)
{
    if (cnt < 8) e &= ((u64)1 << (8 * cnt)) - 1;
    if (at >= 8) r.w[1] |= e << (8 * (at - 8));
    else {
        r.w[0] |= e << (8 * at);
        if (at > 0 && at + cnt > 8) r.w[1] |= e >> (64 - 8 * at);
    }
}

// The run [d0, d0 + 16) of the target pool; total = toff[n], p = the pair of byte d0 (d0 < total)
PG_FN Run target_run(long long d0, long long total, int p, const long long* toff, const TargetSource& src, const uint16_t* tab2)
{
    Run r; r.w[0] = 0; r.w[1] = 0;
    const long long end = d0 + kRun < total ? d0 + kRun : total;
    long long pos = d0;
    while (pos < end) {
        const long long first = toff[p], next = toff[p + 1], stop = next < end ? next : end;
        long long s = (long long)src.pairStart[p] + (pos - first);
        while (pos < stop) {
            const int cnt = stop - pos < 8 ? (int)(stop - pos) : 8;
            put(r, (int)(pos - d0), expand8(codes8(src.pack, src.ndw, s), tab2), cnt);
            pos += cnt; s += cnt;
        }
        ++p;
    }
    return r;
}

// The run [d0, d0 + 16) of the query pool; total = qoff[n], p = the pair of byte d0 (d0 < total)
PG_FN Run query_run(long long d0, long long total, int p, const long long* qoff, const QuerySource& src, const uint8_t* comp)
{
    Run r; r.w[0] = 0; r.w[1] = 0;
    const long long end = d0 + kRun < total ? d0 + kRun : total;
    long long pos = d0;
    while (pos < end) {
        const long long first = qoff[p], next = qoff[p + 1], stop = next < end ? next : end;
        const int q = src.pairQuery[p], strand = src.pairStrand ? (int)src.pairStrand[p] : 0;
        const long long from = src.off[src.stranded ? 2 * (long long)q + strand : q];
        const bool reverse = strand && !src.stranded;
        while (pos < stop) {
            const int cnt = stop - pos < 8 ? (int)(stop - pos) : 8;
            const long long a = pos - first;                      // the pair's bytes a .. a + cnt - 1
            u64 e;
            if (!reverse) e = bytes8(src.pool, src.ndw, from + a);
            else e = revcomp8(bytes8(src.pool, src.ndw, from + (next - first) - a - cnt), cnt, comp);
            put(r, (int)(pos - d0), e, cnt);
            pos += cnt;
        }
        ++p;
    }
    return r;
}

// ---- a target that is resident as its raw bytes (edlibAmdBatchPairsSetSharedWindows: the target pool of a read batch)

// The source of the target pool where the target is bytes: the pool as dwords (ndw of them: what is allocated, reads
// behind them are zero) and per pair the first column of its window
struct TargetBytesSource {
    const u32* bytes; long long ndw;
    const int* pairStart;
};

// the sixteen bytes from byte position s on: the five dwords around them funnel-shifted by the byte phase (two bytes8
// would load six)
PG_FN Run bytes16(const u32* pool, long long ndw, long long s)
{
    const long long i = s >> 2;
    const int sh = 8 * (int)(s & 3);
    const u32 d0 = dword_at(pool, ndw, i), d1 = dword_at(pool, ndw, i + 1), d2 = dword_at(pool, ndw, i + 2),
              d3 = dword_at(pool, ndw, i + 3), d4 = dword_at(pool, ndw, i + 4);
    Run r;
    r.w[0] = (u64)funnel(d0, d1, sh) | (u64)funnel(d1, d2, sh) << 32;
    r.w[1] = (u64)funnel(d2, d3, sh) | (u64)funnel(d3, d4, sh) << 32;
    return r;
}

// The run [d0, d0 + 16) of the target pool from a byte target; total = toff[n], p = the pair of byte d0 (d0 < total).  A
// run inside one pair is one bytes16; a run that meets a pair boundary (or the pool's end) is composed of bytes8 pieces
PG_FN Run target_run_bytes(long long d0, long long total, int p, const long long* toff, const TargetBytesSource& src)
{
    if (toff[p + 1] >= d0 + kRun) return bytes16(src.bytes, src.ndw, (long long)src.pairStart[p] + (d0 - toff[p]));
    Run r; r.w[0] = 0; r.w[1] = 0;
    const long long end = d0 + kRun < total ? d0 + kRun : total;
    long long pos = d0;
    while (pos < end) {
        const long long first = toff[p], next = toff[p + 1], stop = next < end ? next : end;
        long long s = (long long)src.pairStart[p] + (pos - first);
        while (pos < stop) {
            const int cnt = stop - pos < 8 ? (int)(stop - pos) : 8;
            put(r, (int)(pos - d0), bytes8(src.bytes, src.ndw, s), cnt);
            pos += cnt; s += cnt;
        }
        ++p;
    }
    return r;
}

// ---- targets that are resident back to back in one pack (edlibAmdBatchPairsSetCells: the 4-bit pack of a cross batch)

// The source of the target pool where the pack holds many targets, each from a dword of its own: the pack as dwords (ndw of
// them) and per pair the nibble position of its window's first column, 8 * (the target's first dword) + pairStart.  The
// pack may pass 2^31 nibbles: the position is 64 bits wide
struct TargetCellsSource {
    const u32* pack; long long ndw;
    const long long* pairBase;
};

// The nibble position of a window: target t lies at place[t] in the pack's order and starts at dword tdw[place[t]]
PG_FN long long cell_base(const int* place, const long long* tdw, int target, int start)
{
    return 8 * tdw[place[target]] + (long long)start;
}

// The run [d0, d0 + 16) of the target pool from such a pack; total = toff[n], p = the pair of byte d0 (d0 < total)
PG_FN Run target_run_cells(long long d0, long long total, int p, const long long* toff, const TargetCellsSource& src,
                           const uint16_t* tab2)
{
    Run r; r.w[0] = 0; r.w[1] = 0;
    const long long end = d0 + kRun < total ? d0 + kRun : total;
    long long pos = d0;
    while (pos < end) {
        const long long first = toff[p], next = toff[p + 1], stop = next < end ? next : end;
        long long s = src.pairBase[p] + (pos - first);
        while (pos < stop) {
            const int cnt = stop - pos < 8 ? (int)(stop - pos) : 8;
            put(r, (int)(pos - d0), expand8(codes8(src.pack, src.ndw, s), tab2), cnt);
            pos += cnt; s += cnt;
        }
        ++p;
    }
    return r;
}

}  // namespace pairs_gather
}  // namespace edlib_amd
