// cross_kernels_self_strands.hip -- the both-strand self instantiations of the cross scan (cross_scan.hpp, SELF = true and
// STRANDS = true: NW, dense and hit list, 1..8 words, 4 / 8 / 16 symbols) in a translation unit of their own, and the
// strand byte of every sequence's nearest partner (DESIGN.md §4h "Self batches").
#include "cross_scan.hpp"

namespace edlib_amd {

hipError_t launch_scan_cross_self_strands(int nwords, int syms, bool hits, const CrossScanArgs& a, hipStream_t stream)
{
    if (a.numItems == 0) return hipSuccess;
    const int st = cross_scan_args_state(syms, 0, hits, a);
    if (st) return st > 0 ? hipSuccess : hipErrorInvalidValue;
    if (a.numItems < 0 || !a.items || !a.qrank || (!hits && !a.ed)) return hipErrorInvalidValue;
    // mates are neighbouring lanes: an even tile width, and somewhere to put the strand bytes
    if ((a.qt & 1) || !a.strand) return hipErrorInvalidValue;
    return hits ? launch_scan_self_h<true, true>(nwords, syms, a, stream) : launch_scan_self_h<false, true>(nwords, syms, a, stream);
}

// ---------------------------------------------------------------- nearest strand

__global__ void __launch_bounds__(256)
self_nearest_strand_dense_kernel(const uint8_t* __restrict__ pairStrand, const int* __restrict__ nearest, int n,
                                 uint8_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = nearest[i];
    uint8_t v = 0;
    if (j >= 0) {
        const size_t lo = j < i ? j : i, hi = j < i ? i : j;
        v = pairStrand[(size_t)n * lo - (lo * (lo + 1)) / 2 + (hi - lo - 1)];
    }
    out[i] = v;
}

hipError_t launch_self_nearest_strand_dense(const uint8_t* pairStrand, const int* nearest, int n, uint8_t* out,
                                            hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(self_nearest_strand_dense_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       pairStrand, nearest, n, out);
    return hipGetLastError();
}

// the side whose best key is the smaller one is the nearest (self_nearest_hits_kernel): its best hit's byte
__global__ void __launch_bounds__(256)
self_nearest_strand_hits_kernel(const int* __restrict__ best, const uint8_t* __restrict__ bestStrand, int n,
                                uint8_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    const int* up = best;
    const int* down = best + 3 * N;
    const u64 ku = cross_key(up[N + i], up[i]), kd = cross_key(down[N + i], down[i]);
    out[i] = (ku == ~0ull && kd == ~0ull) ? (uint8_t)0 : (ku < kd ? bestStrand[i] : bestStrand[N + i]);
}

hipError_t launch_self_nearest_strand_hits(const int* best, const uint8_t* bestStrand, int n, uint8_t* out,
                                           hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(self_nearest_strand_hits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       best, bestStrand, n, out);
    return hipGetLastError();
}

}  // namespace edlib_amd
