// cross_scan.hpp -- the lane-per-cell scan of cross batches (DESIGN.md "Cross batches"): the kernel template and its
// launch ladders, included by the translation units that instantiate it -- cross_kernels.hip (one strand) and
// cross_kernels_strands.hip (both strands), each half of the cross instantiations, and cross_kernels_self.hip /
// cross_kernels_self_strands.hip (self batches, NW only, one strand / both) and cross_kernels_self_groups.hip (grouped
// self batches, hit list, one strand).
#pragma once
#include "cross_kernels.hpp"
#include "cross_column.hpp"
#include "self_groups_layout.hpp"
#include "strands.hpp"

namespace edlib_amd {

typedef uint32_t u32;
typedef unsigned long long u64;

// ------------------------------------------------------------------- scan

// The column is cross_column<NWD, MODE> (cross_column.hpp, shared with the window kernel).

// HITS: the epilogue appends the cells within k to the hit list (one 64-bit atomicAdd per target-tile step of a wave that
// has any) instead of writing the matrix.  Every lane reaches it with a flag: padding slots and target slots past the end
// take part as non-hits.
// STRANDS: the slots s and s ^ 1 of a query tile hold a query and its reverse complement (qperm = 2 query + strand, qt is
// even), so mates are the lanes l and l ^ 1 of the wave: the same target, `live`, n, query length, NW length window and
// trip count.  Peq staging and the column loop are as for one strand; behind cross_cell_result() the mates exchange their
// records, the even (forward) lane decides by resolve_strands() and is the only one that stores or appends.
// SELF (NW): one set against itself, every unordered pair once (CrossScanArgs::qrank / items).  Block b is
// work item b: a query tile over a run of consecutive target tiles; a lane whose target's rank is not above its query's
// is not live.  The rows are then the shorter sequence of the pair (ranks ascend with the length), a cell is stored at
// the condensed index of its two sequence indices or appended with the key (lower << 32) | higher.
// SELF with STRANDS: a tile of qt slots holds qt / 2 sequences, mates carry the same qrank (so the same `live`), the
// targets are the forward copies; the row sequence is the one that is reverse-complemented, which the host allows only
// where that equals the definition by index (engine_self.hip, complement condition).
// GROUPS (SELF, HITS, one strand; DESIGN.md §4h "Grouped self batches"): the order is (group, length, index), a lane is
// live only where its target's rank is also below qend[slot], the end of its query's group (self_groups_lane(), shared
// with the host layout), and a trip in which no lane of the wave is live is skipped whole.
template <int NWD, int S, int MODE, bool HITS, bool STRANDS, bool SELF = false, bool GROUPS = false>
__global__ void __launch_bounds__(64)
scan_cross_kernel(CrossScanArgs a)
{
    static_assert(!SELF || MODE == 0, "self batches are NW");
    static_assert(!GROUPS || (SELF && HITS && !STRANDS), "grouped self batches are one-strand hit lists");
    __shared__ u32 s_peq[S * NWD * 64];                 // [symbol][word][query of the tile]
    const int lane = threadIdx.x;
    const int qt = a.qt;
    const int slot0 = (SELF ? a.items[3 * blockIdx.x] : (int)blockIdx.x) * qt;
    {
        // staged once: the wave keeps this query tile for all its target tiles
        const u32* src = a.peq + (size_t)(slot0 >> 6) * (S * NWD * 64) + (slot0 & 63);
        for (int i = lane; i < S * NWD * qt; i += 64) {
            const int r = i / qt;
            s_peq[i] = src[r * 64 + (i - r * qt)];
        }
    }
    __syncthreads();
    const int qi = lane & (qt - 1);
    const int ti = lane / qt;
    const int tpt = 64 / qt;
    const int slot = slot0 + qi;
    const int q = a.qperm[slot];
    const int m = a.qlen[slot];
    const int sh = (m - 1) & 31;
    if (!HITS && q < 0) return;                         // (no barrier or ballot below)
    const int rank = SELF ? a.qrank[slot] : 0;
    const int gend = GROUPS ? a.qend[slot] : 0;
    const int ttFirst = SELF ? a.items[3 * blockIdx.x + 1] : (int)blockIdx.y;
    const int ttStep = SELF ? 1 : (int)gridDim.y;
    const int numTT = SELF ? ttFirst + a.items[3 * blockIdx.x + 2] : (a.numSorted + tpt - 1) / tpt;
    for (int tt = ttFirst; tt < numTT; tt += ttStep) {         // wave-uniform trip count
        int ts = tt * tpt + ti;
        bool live = q >= 0 && ts < a.numSorted && (!SELF || ts > rank);
        if (GROUPS) {
            int qiSame;
            live = self_groups_lane(qt, lane, tt, rank, gend, a.numSorted, qiSame, ts);     // (padding: rank = end = -1)
            // wave-uniform, in front of the append every lane reaches: the tile's other runs own this trip
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
        }
        int ed = -1, nloc = 0, end = -1;
        if (live) {
            const int n = a.tlen[ts];
            int score = m, best = 0x7fffffff, cnt = 0, first = -1;
            if (!cross_nw_outside(MODE, a.kcfg, m, n)) {
                const u32* __restrict__ tp = a.tpk + a.tdw[ts];
                u32 Pv[NWD], Mv[NWD];
#pragma unroll
                for (int d = 0; d < NWD; ++d) { Pv[d] = ~0u; Mv[d] = 0u; }
                auto step = [&](u32 c, int j) {
                    cross_column<NWD, MODE>(s_peq + c * (NWD * qt) + qi, qt, Pv, Mv, sh, score);
                    if (MODE != 0) {
                        if (score < best) { best = score; cnt = 1; first = j; }
                        else if (score == best) ++cnt;
                    }
                };
                int j = 0;
                for (; j + 8 <= n; j += 8) {
                    u32 w = tp[j >> 3];
#pragma unroll
                    for (int c = 0; c < 8; ++c) { step(w & 15u, j + c); w >>= 4; }
                }
                if (j < n) {
                    u32 w = tp[j >> 3];
                    for (; j < n; ++j) { step(w & 15u, j); w >>= 4; }
                }
            }
            cross_cell_result(MODE, a.kcfg, m, n, MODE == 0 ? score : best, cnt, first, ed, nloc, end);
        }
        int sbyte = 0;
        if (STRANDS) {
            // every lane that is still here has its mate here: padding slots come in mate pairs (the early return above
            // takes both lanes or neither), and the lanes of a pair left the branch on `live` together
            const int oed = __shfl_xor(ed, 1, 64), onloc = __shfl_xor(nloc, 1, 64), oend = __shfl_xor(end, 1, 64);
            const int w = resolve_strands(ed, oed);
            if (w & kStrandReverse) { ed = oed; nloc = onloc; end = oend; }
            sbyte = w & (kStrandReverse | kStrandBoth);
        }
        const bool mine = !STRANDS || !(q & 1);         // the forward lane reports the pair
        const int qout = STRANDS ? q >> 1 : q;
        if (!HITS) {
            if (SELF) {
                if (live && mine) {
                    // the pair's two sequence indices, lower first
                    const u32 self = (u32)qout, other = (u32)a.tperm[ts];
                    const size_t slo = self < other ? self : other, shi = self < other ? other : self;
                    const size_t at = (size_t)a.numQueries * slo - (slo * (slo + 1)) / 2 + (shi - slo - 1);
                    a.ed[at] = ed;
                    if (STRANDS) a.strand[at] = (uint8_t)sbyte;
                }
                continue;
            }
            if (live && mine) {
                const size_t at = (size_t)a.tperm[ts] * (size_t)a.numQueries + (size_t)qout;
                a.ed[at] = ed; a.nloc[at] = nloc; a.end[at] = end;
                if (STRANDS) a.strand[at] = (uint8_t)sbyte;
            }
            continue;
        }
        // (a wave without a hit issues no atomic: a sparse batch issues almost none)
        const bool hit = live && mine && ed != -1;
        const auto key = [&]() -> u64 {
            const u32 other = (u32)a.tperm[ts];
            // self: the pair's two sequence indices, lower first
            const u32 self = (u32)qout;
            return SELF ? ((u64)(self < other ? self : other) << 32) | (self < other ? other : self) : ((u64)other << 32) | self;
        };
        const u64 at = hit_list_append<3>(a.hits, hit, key, {ed, nloc, end});
        if (STRANDS && at < a.hits.cap) a.strand[at] = (uint8_t)sbyte;
    }
}

// ------------------------------------------------------------- occurrences

// Occurrence batches (DESIGN.md §4h "Occurrence batches"; HW, k >= 0): the tiles, the Peq staging, the column and the
// target walk of scan_cross_kernel, but in place of best / count / first a lane follows its open run of columns scoring
// <= k in registers (rFirst < 0: none; its least score, the first column holding it, how many columns hold it).  A column
// within k opens or extends the run, the first column above k behind it closes it, the end of the target closes the last
// one; closed runs go to the list (hit_list_append<5>: firstEnd, lastEnd, editDistance, endLocation, numLocations) with the
// key (target << 32) | query, among the lanes that are active in the divergent column loop.  A wave none of whose active lanes
// is within k or has a run open pays the compare and one not-taken uniform branch per column; the tracking of the eight
// columns of a target word follows their arithmetic, so that the branches do not cut the column block into eight.  A lane appends its cell's
// runs in ascending column order and the counter only grows: a cell's runs ascend by list index.
template <int NWD, int S>
__global__ void __launch_bounds__(64)
scan_cross_occ_kernel(CrossScanArgs a)
{
    __shared__ u32 s_peq[S * NWD * 64];                 // [symbol][word][query of the tile]
    const int lane = threadIdx.x;
    const int qt = a.qt;
    const int slot0 = (int)blockIdx.x * qt;
    {
        const u32* src = a.peq + (size_t)(slot0 >> 6) * (S * NWD * 64) + (slot0 & 63);
        for (int i = lane; i < S * NWD * qt; i += 64) {
            const int r = i / qt;
            s_peq[i] = src[r * 64 + (i - r * qt)];
        }
    }
    __syncthreads();
    const int qi = lane & (qt - 1);
    const int ti = lane / qt;
    const int tpt = 64 / qt;
    const int slot = slot0 + qi;
    const int q = a.qperm[slot];
    const int m = a.qlen[slot];
    const int sh = (m - 1) & 31;
    const int k = a.kcfg;
    if (q < 0) return;                                  // (no barrier below; the appends are among the active lanes)
    const int numTT = (a.numSorted + tpt - 1) / tpt;
    for (int tt = (int)blockIdx.y; tt < numTT; tt += (int)gridDim.y) {      // wave-uniform trip count
        const int ts = tt * tpt + ti;
        if (ts >= a.numSorted) continue;
        const int n = a.tlen[ts];
        const u64 cell = ((u64)(u32)a.tperm[ts] << 32) | (u32)q;
        const auto key = [&] { return cell; };
        if (m == 0) {                                   // the empty query: one run over a non-empty target, no columns
            hit_list_append<5>(a.hits, n > 0, key, {0, n - 1, 0, 0, n});
            continue;
        }
        const u32* __restrict__ tp = a.tpk + a.tdw[ts];
        u32 Pv[NWD], Mv[NWD];
#pragma unroll
        for (int d = 0; d < NWD; ++d) { Pv[d] = ~0u; Mv[d] = 0u; }
        int score = m, rFirst = -1, rMin = 0, rPos = 0, rCnt = 0;
        auto column = [&](u32 c) { cross_column<NWD, 2>(s_peq + c * (NWD * qt) + qi, qt, Pv, Mv, sh, score); };
        auto track = [&](int sc, int j) {
            const bool in = sc <= k;
            if (__builtin_amdgcn_ballot_w64(in || rFirst >= 0) != 0ull) {       // wave-uniform
                const bool close = !in && rFirst >= 0;
                hit_list_append<5>(a.hits, close, key, {rFirst, j - 1, rMin, rPos, rCnt});
                if (close) rFirst = -1;
                if (in) {
                    if (rFirst < 0) { rFirst = j; rMin = sc; rPos = j; rCnt = 1; }
                    else if (sc < rMin) { rMin = sc; rPos = j; rCnt = 1; }
                    else if (sc == rMin) ++rCnt;
                }
            }
        };
        int j = 0;
        for (; j + 8 <= n; j += 8) {
            // the eight columns of a target word in one straight-line block (their LDS reads issue ahead of the arithmetic,
            // as in scan_cross_kernel), their scores kept; then the compare and branch of each
            u32 w = tp[j >> 3];
            int sc[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) { column(w & 15u); sc[c] = score; w >>= 4; }
#pragma unroll
            for (int c = 0; c < 8; ++c) track(sc[c], j + c);
        }
        if (j < n) {
            u32 w = tp[j >> 3];
            for (; j < n; ++j) { column(w & 15u); track(score, j); w >>= 4; }
        }
        hit_list_append<5>(a.hits, rFirst >= 0, key, {rFirst, n - 1, rMin, rPos, rCnt});     // the run open at the end of the target
    }
}

template <int NWD>
static hipError_t launch_scan_cross_occ_w(int syms, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    const dim3 grid((unsigned)a.numQueryTiles, (unsigned)ysplit);
    if (syms == 4) hipLaunchKernelGGL((scan_cross_occ_kernel<NWD, 4>), grid, dim3(64), 0, stream, a);
    else if (syms == 8) hipLaunchKernelGGL((scan_cross_occ_kernel<NWD, 8>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scan_cross_occ_kernel<NWD, 16>), grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

template <int NWD, int S, bool HITS, bool STRANDS>
static hipError_t launch_scan_cross_ws(int mode, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    const dim3 grid((unsigned)a.numQueryTiles, (unsigned)ysplit);
    if (mode == 0) hipLaunchKernelGGL((scan_cross_kernel<NWD, S, 0, HITS, STRANDS>), grid, dim3(64), 0, stream, a);
    else if (mode == 1) hipLaunchKernelGGL((scan_cross_kernel<NWD, S, 1, HITS, STRANDS>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scan_cross_kernel<NWD, S, 2, HITS, STRANDS>), grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

template <int NWD, bool HITS, bool STRANDS>
static hipError_t launch_scan_cross_w(int syms, int mode, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    if (syms == 4) return launch_scan_cross_ws<NWD, 4, HITS, STRANDS>(mode, a, ysplit, stream);
    if (syms == 8) return launch_scan_cross_ws<NWD, 8, HITS, STRANDS>(mode, a, ysplit, stream);
    return launch_scan_cross_ws<NWD, 16, HITS, STRANDS>(mode, a, ysplit, stream);
}

template <bool HITS, bool STRANDS>
static hipError_t launch_scan_cross_h(int nwords, int syms, int mode, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    switch (nwords) {
    case 1: return launch_scan_cross_w<1, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 2: return launch_scan_cross_w<2, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 3: return launch_scan_cross_w<3, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 4: return launch_scan_cross_w<4, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 5: return launch_scan_cross_w<5, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 6: return launch_scan_cross_w<6, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 7: return launch_scan_cross_w<7, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    case 8: return launch_scan_cross_w<8, HITS, STRANDS>(syms, mode, a, ysplit, stream);
    default: return hipErrorInvalidValue;
    }
}

// the self ladder: one block per work item
template <int NWD, bool HITS, bool STRANDS>
static hipError_t launch_scan_self_w(int syms, const CrossScanArgs& a, hipStream_t stream)
{
    const dim3 grid((unsigned)a.numItems);
    if (syms == 4) hipLaunchKernelGGL((scan_cross_kernel<NWD, 4, 0, HITS, STRANDS, true>), grid, dim3(64), 0, stream, a);
    else if (syms == 8) hipLaunchKernelGGL((scan_cross_kernel<NWD, 8, 0, HITS, STRANDS, true>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scan_cross_kernel<NWD, 16, 0, HITS, STRANDS, true>), grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

template <bool HITS, bool STRANDS>
static hipError_t launch_scan_self_h(int nwords, int syms, const CrossScanArgs& a, hipStream_t stream)
{
    switch (nwords) {
    case 1: return launch_scan_self_w<1, HITS, STRANDS>(syms, a, stream);
    case 2: return launch_scan_self_w<2, HITS, STRANDS>(syms, a, stream);
    case 3: return launch_scan_self_w<3, HITS, STRANDS>(syms, a, stream);
    case 4: return launch_scan_self_w<4, HITS, STRANDS>(syms, a, stream);
    case 5: return launch_scan_self_w<5, HITS, STRANDS>(syms, a, stream);
    case 6: return launch_scan_self_w<6, HITS, STRANDS>(syms, a, stream);
    case 7: return launch_scan_self_w<7, HITS, STRANDS>(syms, a, stream);
    case 8: return launch_scan_self_w<8, HITS, STRANDS>(syms, a, stream);
    default: return hipErrorInvalidValue;
    }
}

// the checks every launcher makes before its ladder; 1: nothing to launch, -1: bad arguments
static inline int cross_scan_args_state(int syms, int mode, bool hits, const CrossScanArgs& a)
{
    if (a.numQueryTiles == 0 || a.numSorted == 0) return 1;
    if ((syms != 4 && syms != 8 && syms != 16) || mode < 0 || mode > 2 || a.qt < 1 || a.qt > 64 || (64 % a.qt) != 0)
        return -1;
    if (hits && (!a.hits.count || !a.hits.key || !a.hits.val)) return -1;
    return 0;
}

}  // namespace edlib_amd
