// strands.hip -- the three kernels of a both-strand read batch (strands.hpp): the reverse-complemented
// query pool, the decision per mate pair, and the gather of the winners into read order.
#include "strands.hpp"

#include <vector>

namespace edlib_amd {

// A wave per read: lane j copies byte j and writes the complement of byte m - 1 - j (both loads hit the lines the wave
// has just read; the pool is made once per batch, at Create).
__global__ void __launch_bounds__(256)
strand_pool_kernel(const uint8_t* __restrict__ in, const long long* __restrict__ off2, int numReads, uint8_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= numReads) return;
    const long long fwd = off2[2 * i], rev = off2[2 * i + 1];
    const long long m = rev - fwd;
    const uint8_t* src = in + (fwd >> 1);
    for (long long j = lane; j < m; j += 64) {
        out[fwd + j] = src[j];
        out[rev + j] = complement_byte(src[m - 1 - j]);
    }
}

hipError_t launch_strand_pool(const uint8_t* in, const long long* off2, int numReads, uint8_t* out, hipStream_t stream)
{
    if (numReads <= 0) return hipSuccess;
    hipLaunchKernelGGL(strand_pool_kernel, dim3((unsigned)((numReads + 3) / 4)), dim3(256), 0, stream, in, off2, numReads, out);
    return hipGetLastError();
}

int make_strand_pool(const char* queries, const long long* off, int nq, DevBuf<uint8_t>& d_pool, DevBuf<long long>& d_off,
                     hipStream_t stream)
{
    const long long bytes = off[nq];
    std::vector<long long> off2(2 * (size_t)nq + 1);
    for (int i = 0; i < nq; ++i) { off2[2 * i] = 2 * off[i]; off2[2 * i + 1] = off[i] + off[i + 1]; }
    off2[2 * (size_t)nq] = 2 * bytes;
    DevBuf<uint8_t> d_raw;
    EDLIB_AMD_HIP(d_raw.alloc((size_t)bytes + 16));
    EDLIB_AMD_HIP(d_pool.alloc(2 * (size_t)bytes + 16)); EDLIB_AMD_HIP(d_off.alloc(2 * (size_t)nq + 1));
    if (bytes) EDLIB_AMD_HIP(hipMemcpy(d_raw.p, queries, (size_t)bytes, hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(hipMemcpy(d_off.p, off2.data(), off2.size() * sizeof(long long), hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(launch_strand_pool(d_raw.p, d_off.p, nq, d_pool.p, stream));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream));                // d_raw dies here
    return 0;
}

__device__ __forceinline__ int slot_distance(int best, int total, int mode, int k)
{
    if (mode == 0) return (best < 0 || (k >= 0 && best > k)) ? -1 : best;
    return total > 0 ? best : -1;
}

__global__ void __launch_bounds__(256)
resolve_strands_kernel(const int* __restrict__ perm, const int* __restrict__ best, const int* __restrict__ total, int npairs,
                       int mode, int k, int* __restrict__ win)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    const int s = 2 * p;
    int w = kStrandNone;
    if (perm[s] >= 0) w = resolve_strands(slot_distance(best[s], total[s], mode, k), slot_distance(best[s + 1], total[s + 1], mode, k));
    win[p] = w;
}

hipError_t launch_resolve_strands(const int* perm, const int* best, const int* total, int nslots, int mode, int k, int* win,
                                  hipStream_t stream)
{
    const int npairs = nslots / 2;
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(resolve_strands_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, stream, perm, best, total,
                       npairs, mode, k, win);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256)
gather_group_strands_kernel(const int* __restrict__ perm, int nslots, const int* __restrict__ win, const int* __restrict__ best,
                            const int* __restrict__ total, const int* __restrict__ qlen, const int* __restrict__ extra,
                            const int* __restrict__ pos, int posCap, int* __restrict__ uScore, int* __restrict__ uCount,
                            int* __restrict__ uQlen, int* __restrict__ uAlpha, int* __restrict__ uPos,
                            uint8_t* __restrict__ uStrand, uint8_t* __restrict__ uBoth)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int u = perm[s];
    if (u < 0) return;
    const int w = win[s >> 1];
    if ((w & kStrandReverse) != (s & 1)) return;                    // the mate is reported
    const int r = u >> 1;
    // (a pair without an alignment reports its forward record as it is: flat_results.hip applies k to it as to any unit)
    uScore[r] = best[s]; uCount[r] = total[s]; uQlen[r] = qlen[s]; uAlpha[r] = extra[s];
    uStrand[r] = (uint8_t)(w & kStrandReverse); uBoth[r] = (w & kStrandBoth) ? 1 : 0;
    for (int i = 0; i < posCap; ++i) uPos[(size_t)r * posCap + i] = pos[(size_t)s * posCap + i];
}

hipError_t launch_gather_group_strands(const int* perm, int nslots, const int* win, const int* best, const int* total,
                                       const int* qlen, const int* extra, const int* pos, int posCap, int* uScore, int* uCount,
                                       int* uQlen, int* uAlpha, int* uPos, uint8_t* uStrand, uint8_t* uBoth, hipStream_t stream)
{
    if (nslots <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_group_strands_kernel, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, stream, perm, nslots,
                       win, best, total, qlen, extra, pos, posCap, uScore, uCount, uQlen, uAlpha, uPos, uStrand, uBoth);
    return hipGetLastError();
}

}  // namespace edlib_amd
