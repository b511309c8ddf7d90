// cross_targets.hip -- a target set of a cross batch prepared on the device (DESIGN.md §4h "Streamed targets"): from the
// raw pool and the caller's offsets as they were uploaded, the rebased offsets and lengths, the 256-bit presence set of
// the pool (census), the targets in the stable order (length, index) by rocPRIM's radix sort and the dword offset of
// every packed target by its exclusive scan.  The pack itself is launch_pack_cross_targets.  A translation unit of its
// own: rocPRIM's headers are most of its compile time.
#include "cross_kernels.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace edlib_amd {

typedef uint32_t u32;

constexpr unsigned kLenBits = 17;                 // lengths 0..65,536 (kCrossMaxTarget)
static_assert(kCrossMaxTarget < (1 << kLenBits), "the sort looks at the bits of a length only");

// offR[t] = offIn[t] - offIn[0] for t <= n; len[t] and idx[t] = t for t < n
__global__ void __launch_bounds__(256)
cross_target_lengths_kernel(const long long* __restrict__ offIn, int n, long long* __restrict__ offR,
                            u32* __restrict__ len, u32* __restrict__ idx)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t > n) return;
    const long long o = offIn[t];
    offR[t] = o - offIn[0];
    if (t < n) { len[t] = (u32)(offIn[t + 1] - o); idx[t] = (u32)t; }
}

// presence[b >> 5] bit (b & 31) for every byte b of the pool.  One wave per target like the pack: a lane keeps the set
// of its bytes in eight dwords, the wave ORs them over its lanes, the block over its four waves, and a dword goes to
// memory by one atomic OR -- only where it has a bit memory does not show yet, which is a handful of blocks of a launch.
__global__ void __launch_bounds__(256)
cross_target_census_kernel(const uint8_t* __restrict__ raw, const long long* __restrict__ off, int n,
                           u32* __restrict__ presence)
{
    __shared__ u32 s_set[4][8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    u32 set[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t < n) {
        const long long o = off[t];
        const int len = (int)(off[t + 1] - o);
        for (int j = lane; j < len; j += 64) {
            const u32 b = raw[o + j];
            const u32 bit = 1u << (b & 31);
#pragma unroll
            for (int d = 0; d < 8; ++d) set[d] |= (b >> 5) == (u32)d ? bit : 0u;
        }
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        u32 v = set[d];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v |= __shfl_xor(v, s, 64);
        if (lane == 0) s_set[wave][d] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const u32 v = s_set[0][threadIdx.x] | s_set[1][threadIdx.x] | s_set[2][threadIdx.x] | s_set[3][threadIdx.x];
        // (a stale read only costs an atomic that changes nothing)
        if (v & ~__hip_atomic_load(presence + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicOr(presence + threadIdx.x, v);
    }
}

// dw[i] = dwords of the packed target of length len[i]
__global__ void __launch_bounds__(256)
cross_target_dwords_kernel(const u32* __restrict__ len, int n, long long* __restrict__ dw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dw[i] = (long long)((len[i] + 7) >> 3);
}

hipError_t cross_targets_order_bytes(int n, size_t* bytes)
{
    *bytes = 0;
    if (n <= 0) return hipSuccess;
    size_t a = 0, b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, a, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr,
                                             (u32*)nullptr, (size_t)n, 0u, kLenBits);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, b, (const long long*)nullptr, (long long*)nullptr, 0LL, (size_t)n,
                                rocprim::plus<long long>());
    *bytes = a > b ? a : b;
    return e;
}

hipError_t launch_cross_targets_prepare(const uint8_t* raw, const long long* offIn, int n, long long* offR, u32* presence,
                                        u32* len, u32* idx, int* tlen, int* tperm, long long* dw, long long* tdw,
                                        void* tmp, size_t tmpBytes, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(presence, 0, 8 * sizeof(u32), stream);
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(cross_target_lengths_kernel, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, stream, offIn, n, offR, len,
                       idx);
    hipLaunchKernelGGL(cross_target_census_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, raw, offR, n,
                       presence);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = tmpBytes;
    e = rocprim::radix_sort_pairs(tmp, bytes, (const u32*)len, reinterpret_cast<u32*>(tlen), (const u32*)idx,
                                  reinterpret_cast<u32*>(tperm), (size_t)n, 0u, kLenBits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cross_target_dwords_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const u32*>(tlen), n, dw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = tmpBytes;
    return rocprim::exclusive_scan(tmp, bytes, (const long long*)dw, tdw, 0LL, (size_t)n, rocprim::plus<long long>(), stream);
}

}  // namespace edlib_amd
