// flat_pairs_prepare.hip -- a flat pair set prepared on the device (DESIGN.md §4b "Streamed pairs"): from the pools and
// the rebased offsets as they were uploaded, the 256-bit presence set of the target pool (census), the Peq offsets, op
// slots and store bases by rocPRIM's exclusive scans, the phase-1 descriptor of every pair (flat_desc: the one definition
// the host's overflow rescan shares), the reversed-query descriptors of the HW start scans and the word-steps of a run.
// Create of a flat set and edlibAmdBatchPairsSetPairs both come here.  A translation unit of its own: rocPRIM's headers
// are most of its compile time.
#include "flat_pairs_prepare.hpp"

#include <rocprim/device/device_scan.hpp>

namespace edlib_amd {

typedef uint32_t u32;

// presence[b >> 5] bit (b & 31) for every byte b of the pool (cross_targets.hip's census over one flat pool: a thread
// takes 16 bytes at a time): a lane keeps the set of its bytes in eight dwords, the wave ORs them over its lanes, the
// block over its four waves, and a dword goes to memory by one atomic OR -- only where it has a bit memory does not show.
__global__ void __launch_bounds__(256)
flat_census_kernel(const uint8_t* __restrict__ pool, const long long bytes, u32* __restrict__ presence)
{
    __shared__ u32 s_set[4][8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u32 set[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long long chunks = (bytes + 15) >> 4;                  // (the pool is 16-byte aligned and padded by 16 bytes)
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (long long)gridDim.x * 256) {
        const uint4 v = *reinterpret_cast<const uint4*>(pool + (c << 4));
        const u32 d[4] = {v.x, v.y, v.z, v.w};
        const int live = bytes - (c << 4) >= 16 ? 16 : (int)(bytes - (c << 4));
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const u32 b = (d[j >> 2] >> (8 * (j & 3))) & 0xffu;
            const u32 bit = j < live ? 1u << (b & 31) : 0u;
#pragma unroll
            for (int w = 0; w < 8; ++w) set[w] |= (b >> 5) == (u32)w ? bit : 0u;
        }
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        u32 v = set[w];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v |= __shfl_xor(v, s, 64);
        if (lane == 0) s_set[wave][w] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const u32 v = s_set[0][threadIdx.x] | s_set[1][threadIdx.x] | s_set[2][threadIdx.x] | s_set[3][threadIdx.x];
        // (a stale read only costs an atomic that changes nothing)
        if (v & ~__hip_atomic_load(presence + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicOr(presence + threadIdx.x, v);
    }
}

// target of unit u: its own, or the one every unit shares
__device__ static inline long long flat_target(const FlatPrepareArgs& a, int u, int& T)
{
    const int at = a.sharedTarget ? 0 : u;
    const long long to = a.toff[at];
    T = (int)(a.toff[at + 1] - to);
    return to;
}

__device__ static inline int flat_sigma(const u32* __restrict__ presence)
{
    int s = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) s += __popc(presence[w]);
    return s;
}

// what the three scans add up, per pair: Peq words, op bytes, store entries; entry n is 0, so that the scans end on the sums
__global__ void __launch_bounds__(256)
flat_sizes_kernel(const FlatPrepareArgs a)
{
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u > a.n) return;
    long long* const peq = a.sizes; long long* const ops = a.sizes + (a.n + 1); long long* const store = a.sizes + 2 * (size_t)(a.n + 1);
    if (u == a.n) { peq[u] = 0; if (a.paths) { ops[u] = 0; store[u] = 0; } return; }
    const int sigmaT = flat_sigma(a.presence);
    int T;
    (void)flat_target(a, u, T);
    const int m = (int)(a.qoff[u + 1] - a.qoff[u]);
    peq[u] = (long long)((m + 63) >> 6) * sigmaT;
    if (a.iota) a.iota[u] = u;
    if (!a.paths) return;
    const int w = flat_window(a.shape.scanMode, m, T);
    const bool ring32 = flat_uses_ring32(true, a.shape.nwStore != 0, a.store32Bytes, a.shape.g32, sigmaT, a.maxWords);
    ops[u] = (long long)m + w + 8;
    store[u] = ring32 ? ring32_store_entries(a.shape.g32, m, w) : ring_store_entries(a.shape.ring, m, w);
}

__global__ void __launch_bounds__(256)
flat_descs_kernel(const FlatPrepareArgs a)
{
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= a.n) return;
    const int sigmaT = flat_sigma(a.presence);
    FlatShape s = a.shape;
    s.ring32 = flat_uses_ring32(a.paths != 0, s.nwStore != 0, a.store32Bytes, s.g32, sigmaT, a.maxWords) ? 1 : 0;
    int T;
    const long long qo = a.qoff[u], to = flat_target(a, u, T);
    PairDesc x = flat_desc(s, u, qo, (int)(a.qoff[u + 1] - qo), to, T, a.peqOff[u]);
    if (a.paths) {
        // the ring32 NW store runs chunk by chunk: bases relative to the chunk's first unit (a handful of cut points)
        long long base = a.storeCum[u];
        if (s.ring32 && s.nwStore) {
            int c = 0;
            while (c + 1 < a.ncuts && a.cuts[c + 1] <= u) ++c;
            base -= a.storeCum[a.cuts[c]];
        }
        a.storeBase[u] = base;
        if (s.nwStore) x.storeOff = base;                        // the phase-1 descriptors ARE the storing scans
    }
    a.descs[u] = x;
    if (a.starts) {
        // reversed-query Peq rows: same layout as the forward ones, behind them (peqOff[n] = all forward words)
        PairDesc r = x;
        r.qoff = x.qoff + x.qlen - 1; r.qstep = -1; r.peqOff = a.peqOff[a.n] + x.peqOff;
        a.revDescs[u] = r;
    }
}

hipError_t flat_prepare_tmp_bytes(int n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const long long*)nullptr, (long long*)nullptr, 0LL, (size_t)n + 1,
                                   rocprim::plus<long long>());
}

hipError_t launch_flat_prepare(const FlatPrepareArgs& a, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(a.steps, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (a.tpool) {
        if ((e = hipMemsetAsync(a.presence, 0, 8 * sizeof(u32), stream)) != hipSuccess) return e;
        const long long chunks = (a.tbytes + 15) >> 4;
        if (chunks > 0) {
            const long long blocks = (chunks + 255) / 256;
            hipLaunchKernelGGL(flat_census_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, a.tpool,
                               a.tbytes, a.presence);
        }
    }
    if (a.n <= 0) return hipGetLastError();
    const unsigned grid = (unsigned)(a.n / 256 + 1);
    const size_t n1 = (size_t)a.n + 1;
    hipLaunchKernelGGL(flat_sizes_kernel, dim3(grid), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    long long* const outs[3] = {a.peqOff, a.opsOff, a.storeCum};
    for (int i = 0; i < (a.paths ? 3 : 1); ++i) {
        size_t bytes = a.tmpBytes;
        e = rocprim::exclusive_scan(a.tmp, bytes, (const long long*)(a.sizes + i * n1), outs[i], 0LL, n1, rocprim::plus<long long>(),
                                    stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(flat_descs_kernel, dim3(grid), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the word-steps of a run over these descriptors never change: counted here, once (both forms of the NW storing scan:
    // which of them runs is known with the census)
    if ((e = launch_count_ring_steps(a.descs, a.n, a.shape.scanMode, 1, a.steps, stream)) != hipSuccess) return e;
    if (a.paths && a.shape.nwStore) e = launch_ring32_word_steps(a.shape.g32, a.descs, a.n, a.steps + 1, stream);
    return e;
}

}  // namespace edlib_amd
