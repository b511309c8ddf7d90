// cross_kernels.hip -- kernels of cross batches (every query against every target, DISTANCE only; DESIGN.md "Cross
// batches").  A lane owns one (query, target) cell and scans the whole height of its query (at most 8 words of 32 rows)
// over its target; a wave is a tile of qt queries x 64 / qt targets, holds the Peq rows of its queries in LDS and strides
// over the target tiles.
#include "cross_scan.hpp"

namespace edlib_amd {

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

// The kernel is scan_cross_kernel (cross_scan.hpp); its both-strand instantiations are in cross_kernels_strands.hip.

hipError_t launch_scan_cross(int nwords, int syms, int mode, bool hits, const CrossScanArgs& a, int ysplit,
                             hipStream_t stream)
{
    const int st = cross_scan_args_state(syms, mode, hits, a);
    if (st) return st > 0 ? hipSuccess : hipErrorInvalidValue;
    return hits ? launch_scan_cross_h<true, false>(nwords, syms, mode, a, ysplit, stream)
                : launch_scan_cross_h<false, false>(nwords, syms, mode, a, ysplit, stream);
}

// -------------------------------------------------------------- best hits

// best2_add / best2_merge: cross_kernels.hpp (shared with the self batches' nearest reduction)

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

// the strand bytes of the best cells (both-strand batches): a gather of the strand matrix at the best indices
__global__ void __launch_bounds__(256)
cross_best_strands_kernel(const uint8_t* __restrict__ cellStrand, int numQueries, int numTargets,
                          const int* __restrict__ bestQ, const int* __restrict__ bestT, uint8_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= numTargets + numQueries) return;
    uint8_t v = 0;
    if (i < numTargets) {
        const int q = bestQ[i];
        if (q >= 0) v = cellStrand[(size_t)i * (size_t)numQueries + (size_t)q];
    } else {
        const int q = i - numTargets, t = bestT[q];
        if (t >= 0) v = cellStrand[(size_t)t * (size_t)numQueries + (size_t)q];
    }
    out[i] = v;
}

hipError_t launch_cross_best_strands(const uint8_t* cellStrand, int numQueries, int numTargets, const int* bestQ,
                                     const int* bestT, uint8_t* out, hipStream_t stream)
{
    const int all = numTargets + numQueries;
    if (all == 0) return hipSuccess;
    hipLaunchKernelGGL(cross_best_strands_kernel, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, stream,
                       cellStrand, numQueries, numTargets, bestQ, bestT, out);
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

__global__ void __launch_bounds__(256)
cross_scatter_bytes_kernel(const long long* __restrict__ cell, const uint8_t* __restrict__ vals, long long n, uint8_t* out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[cell[i]] = vals[i];
}

hipError_t launch_cross_scatter_bytes(const long long* cell, const uint8_t* vals, long long n, uint8_t* out,
                                      hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cross_scatter_bytes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       cell, vals, n, out);
    return hipGetLastError();
}

}  // namespace edlib_amd
