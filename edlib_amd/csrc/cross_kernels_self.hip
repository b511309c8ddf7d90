// cross_kernels_self.hip -- the self instantiations of the cross scan (cross_scan.hpp, SELF = true: NW, one strand, dense
// and hit list, 1..8 words, 4 / 8 / 16 symbols) in a translation unit of their own, and the small kernels of a self
// batch: the nearest other sequence of every sequence, from the condensed vector or from a finished hit list, and the
// scatter of distances computed elsewhere (DESIGN.md §4h "Self batches").
#include "cross_scan.hpp"

namespace edlib_amd {

hipError_t launch_scan_cross_self(int nwords, int syms, bool hits, const CrossScanArgs& a, hipStream_t stream)
{
    if (a.numItems == 0) return hipSuccess;
    const int st = cross_scan_args_state(syms, 0, hits, a);
    if (st) return st > 0 ? hipSuccess : hipErrorInvalidValue;
    if (a.numItems < 0 || !a.items || !a.qrank || (!hits && !a.ed)) return hipErrorInvalidValue;
    return hits ? launch_scan_self_h<true, false>(nwords, syms, a, stream) : launch_scan_self_h<false, false>(nwords, syms, a, stream);
}

// ---------------------------------------------------------------- nearest

// one block per sequence i over its n - 1 partners: the row of the triangle (j > i, consecutive) and the column above it
// (j < i, one cell per row)
__global__ void __launch_bounds__(256)
self_nearest_dense_kernel(const int* __restrict__ ed, int n, int* __restrict__ out)
{
    __shared__ CrossBest2 s_part[4];
    const int i = blockIdx.x;
    const size_t N = (size_t)n;
    CrossBest2 r{~0ull, ~0ull};
    for (int j = threadIdx.x; j < n; j += 256) {
        if (j == i) continue;
        const size_t lo = j < i ? j : i, hi = j < i ? i : j;
        best2_add(r, cross_key(ed[N * lo - (lo * (lo + 1)) / 2 + (hi - lo - 1)], j));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        CrossBest2 x;
        x.b = __shfl_xor(r.b, o, 64);
        x.s = __shfl_xor(r.s, o, 64);
        // the partner lane may hold the same best key only when both are ~0: keys of different j differ
        best2_merge(r, x);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best2_merge(r, s_part[w]);
        best2_store(r, out, out + N, out + 2 * N, i);
    }
}

hipError_t launch_self_nearest_dense(const int* ed, int n, int* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(self_nearest_dense_kernel, dim3((unsigned)n), dim3(256), 0, stream, ed, n, out);
    return hipGetLastError();
}

// best [3][n] over the partners above i (index, distance, second distance), then [3][n] over the partners below: the
// smaller key of the two sides is the nearest; the second distance is the smallest of the other side's best and the two
// sides' seconds
__global__ void __launch_bounds__(256)
self_nearest_hits_kernel(const int* __restrict__ best, int n, int* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    const int* up = best;
    const int* down = best + 3 * N;
    const u64 ku = cross_key(up[N + i], up[i]), kd = cross_key(down[N + i], down[i]);
    CrossBest2 r{ku < kd ? ku : kd, ku < kd ? kd : ku};
    // (only distances of the seconds are known: their index half does not matter to the result)
    const u64 su = cross_key(up[2 * N + i], 0), sd = cross_key(down[2 * N + i], 0);
    if (su < r.s) r.s = su;
    if (sd < r.s) r.s = sd;
    best2_store(r, out, out + N, out + 2 * N, i);
}

hipError_t launch_self_nearest_hits(const int* best, int n, int* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(self_nearest_hits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, best, n, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- scatter

__global__ void __launch_bounds__(256)
self_scatter_kernel(const long long* __restrict__ cell, const int* __restrict__ vals, long long n, int* __restrict__ ed)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ed[cell[i]] = vals[i];
}

hipError_t launch_self_scatter(const long long* cell, const int* vals, long long n, int* ed, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(self_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cell, vals, n, ed);
    return hipGetLastError();
}

}  // namespace edlib_amd
