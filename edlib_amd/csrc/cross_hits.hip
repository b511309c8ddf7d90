// cross_hits.hip -- the hit list of a cross batch finished on the device (DESIGN.md "Cross batches", Hits): the settled
// list (hit_list.hpp: the scan's hits and those of the internal sessions behind them) sorted by (target << 32) | query,
// gathered into CSR order with its target offsets, and -- the cross batch's own -- the best hits reduced from the list.
#include "cross_kernels.hpp"

namespace edlib_amd {

typedef uint32_t u32;
typedef unsigned long long u64;

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

hipError_t launch_cross_hits_finish(HitListBuffers& hl, int numQueries, int numTargets, u64* bkey, int* best,
                                    uint8_t* bestStrand, hipStream_t stream)
{
    hipError_t e = hl.sort(numTargets, stream);
    if (e == hipSuccess) e = hl.gather(stream);
    if (e == hipSuccess) e = hl.offsets(stream);
    if (e != hipSuccess) return e;
    const long long n = hl.n;
    const u64* key = hl.key.p;
    const int* val = hl.val.p;
    const uint8_t* strand = bestStrand ? hl.byte.p : nullptr;
    const unsigned nb = (unsigned)((n + 255) / 256);
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

hipError_t launch_cross_occ_finish(HitListBuffers& hl, int numTargets, hipStream_t stream)
{
    hipError_t e = hl.sort(numTargets, stream);
    if (e == hipSuccess) e = hl.gather(stream);
    if (e == hipSuccess) e = hl.offsets(stream);
    return e;
}

}  // namespace edlib_amd
