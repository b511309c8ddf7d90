// cross_kernels.hip -- kernels of cross batches (every query against every target, DISTANCE only; DESIGN.md "Cross
// batches").  A lane owns one (query, target) cell and scans the whole height of its query (at most 8 words of 32 rows)
// over its target; a wave is a tile of qt queries x 64 / qt targets, holds the Peq rows of its queries in LDS and strides
// over the target tiles.
#include "cross_kernels.hpp"
#include "cross_column.hpp"

namespace edlib_amd {

typedef uint32_t u32;
typedef unsigned long long u64;

// ------------------------------------------------------------- target pack

// Target pool in sorted order, 4-bit symbol codes (tlut), 8 columns per dword, LSB first, each target from a dword
// boundary (the cross form of launch_pack_target_2bit).  One wave per target.
__global__ void __launch_bounds__(256)
pack_cross_targets_kernel(const uint8_t* __restrict__ raw, const long long* __restrict__ toff,
                          const int* __restrict__ tperm, const long long* __restrict__ tdw, int numSorted,
                          const uint8_t* __restrict__ tlut, u32* __restrict__ tpk)
{
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = tlut[threadIdx.x];
    __syncthreads();
    const int ts = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ts >= numSorted) return;
    const int t = tperm[ts];
    const long long off = toff[t];
    const int n = (int)(toff[t + 1] - off);
    const long long base = tdw[ts];
    for (int w = threadIdx.x & 63; w * 8 < n; w += 64) {
        u32 v = 0;
        for (int c = 0; c < 8; ++c) {
            const int j = w * 8 + c;
            if (j < n) v |= (u32)(s_lut[raw[off + j]] & 15) << (4 * c);
        }
        tpk[base + w] = v;
    }
}

hipError_t launch_pack_cross_targets(const uint8_t* raw, const long long* toff, const int* tperm, const long long* tdw,
                                     int numSorted, const uint8_t* tlut, u32* tpk, hipStream_t stream)
{
    if (numSorted == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_cross_targets_kernel, dim3((unsigned)((numSorted + 3) / 4)), dim3(256), 0, stream,
                       raw, toff, tperm, tdw, numSorted, tlut, tpk);
    return hipGetLastError();
}

// ------------------------------------------------------------------- scan

// The column is cross_column<NWD, MODE> (cross_column.hpp, shared with the window kernel).

// HITS: the epilogue appends the cells within k to the hit list (one 64-bit atomicAdd per target-tile step of a wave that
// has any) instead of writing the matrix.  Every lane reaches it with a flag: padding slots and target slots past the end
// take part as non-hits.
template <int NWD, int S, int MODE, bool HITS>
__global__ void __launch_bounds__(64)
scan_cross_kernel(CrossScanArgs a)
{
    __shared__ u32 s_peq[S * NWD * 64];                 // [symbol][word][query of the tile]
    const int lane = threadIdx.x;
    const int qt = a.qt;
    const int slot0 = blockIdx.x * qt;
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
    const int numTT = (a.numSorted + tpt - 1) / tpt;
    for (int tt = blockIdx.y; tt < numTT; tt += gridDim.y) {   // wave-uniform trip count
        const int ts = tt * tpt + ti;
        const bool live = q >= 0 && ts < a.numSorted;
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
        if (!HITS) {
            if (live) {
                const size_t at = (size_t)a.tperm[ts] * (size_t)a.numQueries + (size_t)q;
                a.ed[at] = ed; a.nloc[at] = nloc; a.end[at] = end;
            }
            continue;
        }
        const bool hit = live && ed != -1;
        const u64 mask = __ballot(hit);
        if (mask == 0) continue;                        // a sparse batch issues almost no atomics
        const int leader = __ffsll((long long)mask) - 1;    // a lane with a hit: active
        u64 base = 0;
        if (lane == leader) base = atomicAdd(a.hitCount, (u64)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (hit) {
            const u64 at = base + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
            if (at < a.hitCap) {
                a.hitKey[at] = ((u64)(u32)a.tperm[ts] << 32) | (u32)q;
                a.hitVal[at] = ed; a.hitVal[a.hitCap + at] = nloc; a.hitVal[2 * a.hitCap + at] = end;
            }
        }
    }
}

template <int NWD, int S, bool HITS>
static hipError_t launch_scan_cross_ws(int mode, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    const dim3 grid((unsigned)a.numQueryTiles, (unsigned)ysplit);
    if (mode == 0) hipLaunchKernelGGL((scan_cross_kernel<NWD, S, 0, HITS>), grid, dim3(64), 0, stream, a);
    else if (mode == 1) hipLaunchKernelGGL((scan_cross_kernel<NWD, S, 1, HITS>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scan_cross_kernel<NWD, S, 2, HITS>), grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

template <int NWD, bool HITS>
static hipError_t launch_scan_cross_w(int syms, int mode, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    if (syms == 4) return launch_scan_cross_ws<NWD, 4, HITS>(mode, a, ysplit, stream);
    if (syms == 8) return launch_scan_cross_ws<NWD, 8, HITS>(mode, a, ysplit, stream);
    return launch_scan_cross_ws<NWD, 16, HITS>(mode, a, ysplit, stream);
}

template <bool HITS>
static hipError_t launch_scan_cross_h(int nwords, int syms, int mode, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    switch (nwords) {
    case 1: return launch_scan_cross_w<1, HITS>(syms, mode, a, ysplit, stream);
    case 2: return launch_scan_cross_w<2, HITS>(syms, mode, a, ysplit, stream);
    case 3: return launch_scan_cross_w<3, HITS>(syms, mode, a, ysplit, stream);
    case 4: return launch_scan_cross_w<4, HITS>(syms, mode, a, ysplit, stream);
    case 5: return launch_scan_cross_w<5, HITS>(syms, mode, a, ysplit, stream);
    case 6: return launch_scan_cross_w<6, HITS>(syms, mode, a, ysplit, stream);
    case 7: return launch_scan_cross_w<7, HITS>(syms, mode, a, ysplit, stream);
    case 8: return launch_scan_cross_w<8, HITS>(syms, mode, a, ysplit, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_cross(int nwords, int syms, int mode, bool hits, const CrossScanArgs& a, int ysplit,
                             hipStream_t stream)
{
    if (a.numQueryTiles == 0 || a.numSorted == 0) return hipSuccess;
    if ((syms != 4 && syms != 8 && syms != 16) || mode < 0 || mode > 2 || a.qt < 1 || a.qt > 64 || (64 % a.qt) != 0)
        return hipErrorInvalidValue;
    if (hits && (!a.hitCount || !a.hitKey || !a.hitVal)) return hipErrorInvalidValue;
    return hits ? launch_scan_cross_h<true>(nwords, syms, mode, a, ysplit, stream)
                : launch_scan_cross_h<false>(nwords, syms, mode, a, ysplit, stream);
}

// -------------------------------------------------------------- best hits

__device__ __forceinline__ void best2_add(CrossBest2& r, const u64 key)
{
    if (key < r.b) { r.s = r.b; r.b = key; }
    else if (key < r.s) r.s = key;
}

__device__ __forceinline__ void best2_merge(CrossBest2& r, const CrossBest2& o)
{
    if (o.b < r.b) { r.s = r.b < o.s ? r.b : o.s; r.b = o.b; }
    else { r.s = r.s < o.b ? r.s : o.b; }
}

// per target over its queries: one wave per row of the matrix
__global__ void __launch_bounds__(256)
cross_best_rows_kernel(const int* __restrict__ ed, int numQueries, int numTargets, int* bestQ, int* bestQD, int* secondQD)
{
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= numTargets) return;
    const int* row = ed + (size_t)t * (size_t)numQueries;
    CrossBest2 r{~0ull, ~0ull};
    for (int q = lane; q < numQueries; q += 64) best2_add(r, cross_key(row[q], q));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        CrossBest2 x;
        x.b = __shfl_xor(r.b, o, 64);
        x.s = __shfl_xor(r.s, o, 64);
        best2_merge(r, x);
    }
    if (lane == 0) best2_store(r, bestQ, bestQD, secondQD, t);
}

// per query over the targets: a lane per query over a chunk of targets (coalesced rows), partials per chunk
__global__ void __launch_bounds__(64)
cross_best_cols_partial_kernel(const int* __restrict__ ed, int numQueries, int numTargets, int targetChunk,
                               CrossBest2* __restrict__ partial)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= numQueries) return;
    const int t0 = blockIdx.y * targetChunk;
    const int t1 = t0 + targetChunk < numTargets ? t0 + targetChunk : numTargets;
    CrossBest2 r{~0ull, ~0ull};
    for (int t = t0; t < t1; ++t) best2_add(r, cross_key(ed[(size_t)t * (size_t)numQueries + q], t));
    partial[(size_t)blockIdx.y * (size_t)numQueries + q] = r;
}

__global__ void __launch_bounds__(256)
cross_best_cols_final_kernel(const CrossBest2* __restrict__ partial, int numQueries, int numChunks,
                             int* bestT, int* bestTD, int* secondTD)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= numQueries) return;
    CrossBest2 r{~0ull, ~0ull};
    for (int c = 0; c < numChunks; ++c) best2_merge(r, partial[(size_t)c * (size_t)numQueries + q]);
    best2_store(r, bestT, bestTD, secondTD, q);
}

hipError_t launch_cross_best(const int* ed, int numQueries, int numTargets,
                             int* bestQ, int* bestQD, int* secondQD, int* bestT, int* bestTD, int* secondTD,
                             CrossBest2* partial, int targetChunk, hipStream_t stream)
{
    if (numTargets > 0)
        hipLaunchKernelGGL(cross_best_rows_kernel, dim3((unsigned)((numTargets + 3) / 4)), dim3(256), 0, stream,
                           ed, numQueries, numTargets, bestQ, bestQD, secondQD);
    if (numQueries > 0) {
        const int chunks = numTargets > 0 ? (numTargets + targetChunk - 1) / targetChunk : 0;
        if (chunks > 0)
            hipLaunchKernelGGL(cross_best_cols_partial_kernel, dim3((unsigned)((numQueries + 63) / 64), (unsigned)chunks),
                               dim3(64), 0, stream, ed, numQueries, numTargets, targetChunk, partial);
        hipLaunchKernelGGL(cross_best_cols_final_kernel, dim3((unsigned)((numQueries + 255) / 256)), dim3(256), 0, stream,
                           partial, numQueries, chunks, bestT, bestTD, secondTD);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------- scatter

__global__ void __launch_bounds__(256)
cross_scatter_kernel(const long long* __restrict__ cell, const int* __restrict__ vals, long long n,
                     int* ed, int* nloc, int* end)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long at = cell[i];
    ed[at] = vals[3 * i]; nloc[at] = vals[3 * i + 1]; end[at] = vals[3 * i + 2];
}

hipError_t launch_cross_scatter(const long long* cell, const int* vals, long long n, int* ed, int* nloc, int* end,
                                hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cross_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       cell, vals, n, ed, nloc, end);
    return hipGetLastError();
}

}  // namespace edlib_amd
