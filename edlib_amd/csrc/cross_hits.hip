// cross_hits.hip -- the hit list of a cross batch finished on the device (DESIGN.md "Cross batches", Hits): the hits the
// scan appended (and those of the internal sessions behind them) sorted by (target << 32) | query with rocPRIM's radix
// sort, gathered into CSR order, the target offsets from the boundaries of the sorted keys, and the best hits reduced
// from the list.  A translation unit of its own: rocPRIM's headers are most of its compile time.
#include "cross_kernels.hpp"

#include <rocprim/device/device_radix_sort.hpp>

namespace edlib_amd {

typedef uint32_t u32;
typedef unsigned long long u64;

// key bits the sort looks at: the query half and as many target bits as numTargets needs
static unsigned key_end_bit(int numTargets)
{
    unsigned b = 0;
    while (b < 31 && (1u << b) < (unsigned)numTargets) ++b;
    return 32 + b;
}

hipError_t cross_hits_sort_bytes(long long n, int numTargets, size_t* bytes)
{
    *bytes = 0;
    if (n <= 0) return hipSuccess;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr,
                                     (u32*)nullptr, (size_t)n, 0u, key_end_bit(numTargets));
}

__global__ void __launch_bounds__(256) cross_hits_iota_kernel(u32* __restrict__ idx, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = (u32)i;
}

hipError_t launch_cross_hits_iota(u32* idx, long long n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cross_hits_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, idx, n);
    return hipGetLastError();
}

// out [4][n]: query, editDistance, numLocations, endLocation of sorted hit i
__global__ void __launch_bounds__(256)
cross_hits_gather_kernel(const u64* __restrict__ skey, const u32* __restrict__ sidx, const int* __restrict__ val,
                         long long cap, long long n, int* __restrict__ out, const uint8_t* __restrict__ strand,
                         uint8_t* __restrict__ strandOut)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long j = sidx[i];
    out[i] = (int)(u32)skey[i];
    out[n + i] = val[j];
    out[2 * n + i] = val[cap + j];
    out[3 * n + i] = val[2 * cap + j];
    if (strand) strandOut[i] = strand[j];
}

// targetOffsets[t] = first sorted hit of target t or later (t = numTargets: n)
__global__ void __launch_bounds__(256)
cross_hits_offsets_kernel(const u64* __restrict__ skey, long long n, int numTargets, long long* __restrict__ toff)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t > numTargets) return;
    const u64 want = (u64)(u32)t << 32;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skey[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    toff[t] = lo;
}

// Best hits from the list, order-free: pass 1 the smallest (distance << 32 | index) key per target (over its queries) and
// per query (over its targets), pass 2 the smallest key that is not the best; bkey = [best][nt + nq], [second][nt + nq].
template <int PASS>
__global__ void __launch_bounds__(256)
cross_hits_best_kernel(const u64* __restrict__ key, const int* __restrict__ ed, long long n, int numTargets,
                       int numQueries, u64* __restrict__ bkey)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    const int t = (int)(k >> 32), q = (int)(u32)k;
    const u64 kq = cross_key(ed[i], q), kt = cross_key(ed[i], t);
    u64* b1 = bkey;
    u64* b2 = bkey + (size_t)numTargets + (size_t)numQueries;
    if (PASS == 1) {
        atomicMin(b1 + t, kq);
        atomicMin(b1 + numTargets + q, kt);
    } else {
        if (kq != b1[t]) atomicMin(b2 + t, kq);
        if (kt != b1[numTargets + q]) atomicMin(b2 + numTargets + q, kt);
    }
}

// both strands: the byte of the hit whose key is the best of its target / of its query (keys differ, so one hit each)
__global__ void __launch_bounds__(256)
cross_hits_best_strands_kernel(const u64* __restrict__ key, const int* __restrict__ ed, const uint8_t* __restrict__ strand,
                               long long n, int numTargets, int numQueries, const u64* __restrict__ bkey,
                               uint8_t* __restrict__ bestStrand)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    const int t = (int)(k >> 32), q = (int)(u32)k;
    if (cross_key(ed[i], q) == bkey[t]) bestStrand[t] = strand[i];
    if (cross_key(ed[i], t) == bkey[numTargets + q]) bestStrand[numTargets + q] = strand[i];
}

__global__ void __launch_bounds__(256)
cross_hits_best_store_kernel(const u64* __restrict__ bkey, int numTargets, int numQueries, int* __restrict__ best)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int all = numTargets + numQueries;
    if (i >= all) return;
    const CrossBest2 r{bkey[i], bkey[all + i]};
    if (i < numTargets) best2_store(r, best, best + numTargets, best + 2 * (size_t)numTargets, i);
    else {
        int* bt = best + 3 * (size_t)numTargets;
        best2_store(r, bt, bt + numQueries, bt + 2 * (size_t)numQueries, i - numTargets);
    }
}

hipError_t launch_cross_hits_finish(const u64* key, const int* val, long long cap, long long n, int numQueries,
                                    int numTargets, const u32* idx, u64* skey, u32* sidx, void* tmp, size_t tmpBytes,
                                    long long* targetOffsets, int* out, u64* bkey, int* best, const uint8_t* strand,
                                    uint8_t* strandOut, uint8_t* bestStrand, hipStream_t stream)
{
    hipError_t e;
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (n > 0) {
        size_t bytes = tmpBytes;
        e = rocprim::radix_sort_pairs(tmp, bytes, key, skey, idx, sidx, (size_t)n, 0u, key_end_bit(numTargets), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cross_hits_gather_kernel, dim3(nb), dim3(256), 0, stream, skey, sidx, val, cap, n, out,
                           strand, strandOut);
    }
    hipLaunchKernelGGL(cross_hits_offsets_kernel, dim3((unsigned)((numTargets + 1 + 255) / 256)), dim3(256), 0, stream,
                       skey, n, numTargets, targetOffsets);
    const int all = numTargets + numQueries;
    if (all == 0) return hipGetLastError();
    e = hipMemsetAsync(bkey, 0xff, 2 * (size_t)all * sizeof(u64), stream);
    if (e != hipSuccess) return e;
    if (strand) {
        e = hipMemsetAsync(bestStrand, 0, (size_t)all, stream);
        if (e != hipSuccess) return e;
    }
    if (n > 0) {
        hipLaunchKernelGGL(cross_hits_best_kernel<1>, dim3(nb), dim3(256), 0, stream, key, val, n, numTargets, numQueries, bkey);
        hipLaunchKernelGGL(cross_hits_best_kernel<2>, dim3(nb), dim3(256), 0, stream, key, val, n, numTargets, numQueries, bkey);
        if (strand)
            hipLaunchKernelGGL(cross_hits_best_strands_kernel, dim3(nb), dim3(256), 0, stream, key, val, strand, n, numTargets,
                               numQueries, bkey, bestStrand);
    }
    hipLaunchKernelGGL(cross_hits_best_store_kernel, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, stream,
                       bkey, numTargets, numQueries, best);
    return hipGetLastError();
}

// out [6][n]: query, firstEnd, lastEnd, editDistance, endLocation, numLocations of sorted run i
__global__ void __launch_bounds__(256)
cross_occ_gather_kernel(const u64* __restrict__ skey, const u32* __restrict__ sidx, const int* __restrict__ val,
                        long long cap, long long n, int* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long j = sidx[i];
    out[i] = (int)(u32)skey[i];
#pragma unroll
    for (int f = 0; f < 5; ++f) out[(f + 1) * n + i] = val[f * cap + j];
}

hipError_t launch_cross_occ_finish(const u64* key, const int* val, long long cap, long long n, int numTargets,
                                   const u32* idx, u64* skey, u32* sidx, void* tmp, size_t tmpBytes,
                                   long long* targetOffsets, int* out, hipStream_t stream)
{
    if (n > 0) {
        size_t bytes = tmpBytes;
        // (a radix sort is stable: equal keys -- the runs of one cell -- keep the order of the list)
        const hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, key, skey, idx, sidx, (size_t)n, 0u, key_end_bit(numTargets), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cross_occ_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, skey, sidx, val,
                           cap, n, out);
    }
    hipLaunchKernelGGL(cross_hits_offsets_kernel, dim3((unsigned)((numTargets + 1 + 255) / 256)), dim3(256), 0, stream,
                       skey, n, numTargets, targetOffsets);
    return hipGetLastError();
}

}  // namespace edlib_amd
