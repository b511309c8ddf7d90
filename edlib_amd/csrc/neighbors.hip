// neighbors.hip -- the K nearest neighbours of every row of a self or cross batch, selected on the device from the
// results where the Run left them (edlibAmdBatchSelfNeighbors, edlibAmdBatchCrossNeighbors, DESIGN.md §4h "Neighbours").
// One selection kernel, a wave per row: the wave keeps the 64 smallest keys it has met, ascending by lane, reads the row
// 64 candidates at a time, skips a chunk that cannot change the first K behind one ballot, and otherwise sorts the chunk
// across its lanes and merges it into the kept list (the schedule: neighbors_core.hpp).  No LDS, no atomics, no waiting.
// A self hit list holds each pair once, under its lower index: three launches mirror it into a symmetric CSR first.
#include "cross_kernels.hpp"
#include "neighbors_core.hpp"

#include <rocprim/device/device_scan.hpp>

namespace edlib_amd {

namespace nb = neighbors;
typedef uint32_t u32;
typedef unsigned long long u64;

size_t NeighborsBuffers::ints(int rows, int K)
{
    const size_t cells = (size_t)rows * (size_t)K;
    return (size_t)rows + 2 * cells + (cells + 3) / 4;
}

NeighborsBuffers NeighborsBuffers::carve(int* base, int rows, int K)
{
    NeighborsBuffers b;
    const size_t cells = (size_t)rows * (size_t)K;
    b.count = base; b.neighbor = base + rows; b.distance = b.neighbor + cells;
    b.strand = reinterpret_cast<uint8_t*>(b.distance + cells);
    return b;
}

size_t NeighborsMirror::bytes(int n, long long numHits)
{
    // off [n + 1] long long, then degree [n + 1] and cursor [n] (and a pad), then three planes of 2 numHits
    return ((size_t)n + 1) * sizeof(long long) + (2 * (size_t)n + 2) * sizeof(int) + 6 * (size_t)numHits * sizeof(int);
}

NeighborsMirror NeighborsMirror::carve(uint8_t* base, int n, long long numHits)
{
    NeighborsMirror m;
    m.off = reinterpret_cast<long long*>(base);
    m.degree = reinterpret_cast<int*>(m.off + (size_t)n + 1);
    m.cursor = m.degree + (size_t)n + 1;
    m.partner = m.cursor + (size_t)n + 1;
    m.distance = m.partner + 2 * (size_t)numHits;
    m.position = reinterpret_cast<u32*>(m.distance + 2 * (size_t)numHits);
    return m;
}

// ---------------------------------------------------------------- the exchange

// the value of the lane at `distance`: lane i <-> lane i + 32 is one half exchange of the register with itself (the upper
// half of the first result and the lower half of the second are the other half's values), nearer lanes go through the
// cross-lane network
template <int DISTANCE>
__device__ __forceinline__ u32 from_partner(u32 v, int lane)
{
#if __has_builtin(__builtin_amdgcn_permlane32_swap)
    if (DISTANCE == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return lane < 32 ? r[1] : r[0];
    }
#endif
    return (u32)__shfl_xor((int)v, DISTANCE, 64);
}

template <int DISTANCE>
__device__ __forceinline__ void compare_exchange(u64& key, u32& pay, const bool keepsMin, const int lane)
{
    const u64 other = ((u64)from_partner<DISTANCE>((u32)(key >> 32), lane) << 32) | from_partner<DISTANCE>((u32)key, lane);
    const u32 otherPay = from_partner<DISTANCE>(pay, lane);
    if (nb::takes_partner(keepsMin, key, other)) { key = other; pay = otherPay; }
}

template <int S>
__device__ __forceinline__ void sort_stages(u64& key, u32& pay, const int lane)
{
    if constexpr (S < nb::kSortStages) {
        compare_exchange<nb::sort_distance(S)>(key, pay, nb::sort_keeps_min(S, lane), lane);
        sort_stages<S + 1>(key, pay, lane);
    }
}

template <int S>
__device__ __forceinline__ void merge_stages(u64& key, u32& pay, const int lane)
{
    if constexpr (S < nb::kMergeStages) {
        compare_exchange<nb::merge_distance(S)>(key, pay, nb::merge_keeps_min(S, lane), lane);
        merge_stages<S + 1>(key, pay, lane);
    }
}

__device__ __forceinline__ u64 read_lane(u64 v, int lane)
{
    return ((u64)(u32)__shfl((int)(u32)(v >> 32), lane, 64) << 32) | (u32)__shfl((int)(u32)v, lane, 64);
}

// ---------------------------------------------------------------- the selection

__global__ void __launch_bounds__(nb::kLanes * nb::kRowsPerBlock)
neighbors_select_kernel(const NeighborsSource s, const int K, const int level, const NeighborsBuffers out)
{
    const int lane = threadIdx.x & (nb::kLanes - 1);
    const int row = blockIdx.x * nb::kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= s.numRows) return;                                   // (a whole wave: the branch is uniform)

    long long begin = 0, length = s.rowLength;
    if (s.kind == NeighborsSource::kCsr) { begin = s.off[row]; length = s.off[row + 1] - begin; }

    u64 key = nb::kNoKey;                                            // the kept list, ascending by lane
    u32 pay = 0;
    u64 kth = nb::kNoKey;                                            // the key of lane K - 1: what a newcomer has to beat
    for (long long c0 = 0; c0 < length; c0 += nb::kLanes) {
        const long long c = c0 + lane;
        u64 ck = nb::kNoKey;
        u32 cp = 0;
        if (c < length) {
            if (s.kind == NeighborsSource::kMatrix)
                ck = nb::candidate_key(s.ed[nb::matrix_at(s.rowLength, row, (int)c)], (int)c, level);
            else if (s.kind == NeighborsSource::kCondensed) {
                if ((int)c != row) ck = nb::candidate_key(s.ed[nb::condensed_at(s.rowLength, row, (int)c)], (int)c, level);
            } else {
                const long long e = nb::csr_at(begin, c);
                ck = nb::candidate_key(s.distance[e], s.partner[e], level);
                cp = s.position ? s.position[e] : (u32)e;
            }
        }
        if (!__builtin_amdgcn_ballot_w64(ck < kth)) continue;       // no key of the chunk enters the first K
        sort_stages<0>(ck, cp, lane);
        // the smaller of the kept key and the reversed chunk's: the 64 smallest of both, a bitonic sequence
        const u64 rk = read_lane(ck, nb::reversed_lane(lane));
        const u32 rp = (u32)__shfl((int)cp, nb::reversed_lane(lane), 64);
        if (rk < key) { key = rk; pay = rp; }
        merge_stages<0>(key, pay, lane);
        kth = read_lane(key, K - 1);
    }

    const u64 kept = __builtin_amdgcn_ballot_w64(lane < K && key != nb::kNoKey);
    const int count = nb::reported(K, __popcll(kept));
    if (lane == 0) out.count[row] = count;
    if (lane >= K) return;
    const size_t at = (size_t)row * (size_t)K + (size_t)lane;
    const bool have = lane < count;
    const int index = nb::key_index(key);
    out.neighbor[at] = have ? index : -1;
    out.distance[at] = have ? nb::key_distance(key) : -1;
    if (s.strand) {
        uint8_t byte = 0;
        if (have) {
            const long long p = s.kind == NeighborsSource::kMatrix ? nb::matrix_at(s.rowLength, row, index)
                              : s.kind == NeighborsSource::kCondensed ? nb::condensed_at(s.rowLength, row, index)
                              : (long long)pay;
            byte = s.strand[p];
        }
        out.strand[at] = byte;
    }
}

hipError_t launch_neighbors_select(const NeighborsSource& s, int K, int level, const NeighborsBuffers& out, hipStream_t stream)
{
    if (s.numRows <= 0) return hipSuccess;
    if (K < 1 || K > nb::kMaxK) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((s.numRows + nb::kRowsPerBlock - 1) / nb::kRowsPerBlock);
    hipLaunchKernelGGL(neighbors_select_kernel, dim3(blocks), dim3(nb::kLanes * nb::kRowsPerBlock), 0, stream, s, K, level, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the mirror of a self hit list

// a thread per finished hit (i, j), i < j: the row from the sorted key's high half, as the list's finish leaves it
__global__ void __launch_bounds__(256)
neighbors_degree_kernel(const u64* __restrict__ skey, const int* __restrict__ partner, long long numHits, int* degree)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= numHits) return;
    atomicAdd(degree + (int)(skey[e] >> 32), 1);
    atomicAdd(degree + partner[e], 1);
}

// Hit e goes into the rows of both its ends, at the place the row's cursor hands out.  The order inside a mirrored row
// is therefore whatever the atomics give, and differs from call to call.  The selection does not see it: the keys
// (distance << 32) | partner of a row are unique -- a pair is in the list once --, so the K smallest are one set in one
// order whichever entry is met first, and what is written out is the same bit for bit.
__global__ void __launch_bounds__(256)
neighbors_scatter_kernel(const u64* __restrict__ skey, const int* __restrict__ partner, const int* __restrict__ ed,
                         long long numHits, const long long* __restrict__ off, int* cursor, int* __restrict__ mpartner,
                         int* __restrict__ mdistance, u32* __restrict__ mposition)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= numHits) return;
    const int i = (int)(skey[e] >> 32), j = partner[e], d = ed[e];
    const long long a = off[i] + atomicAdd(cursor + i, 1), b = off[j] + atomicAdd(cursor + j, 1);
    mpartner[a] = j; mdistance[a] = d; mposition[a] = (u32)e;
    mpartner[b] = i; mdistance[b] = d; mposition[b] = (u32)e;
}

hipError_t neighbors_mirror_scratch(int n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const int*)nullptr, (long long*)nullptr, 0LL, (size_t)n + 1,
                                   rocprim::plus<long long>());
}

hipError_t launch_neighbors_mirror(const NeighborsMirror& m, int n, const unsigned long long* skey, const int* partner,
                                   const int* ed, long long numHits, void* scratch, size_t scratchBytes, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    // degree [n + 1] (the last stays 0: the scan's total lands in off[n]) and cursor [n], back to back
    hipError_t e = hipMemsetAsync(m.degree, 0, (2 * (size_t)n + 2) * sizeof(int), stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((numHits + 255) / 256)), block(256);
    if (numHits > 0) hipLaunchKernelGGL(neighbors_degree_kernel, grid, block, 0, stream, skey, partner, numHits, m.degree);
    size_t bytes = scratchBytes;
    e = rocprim::exclusive_scan(scratch, bytes, (const int*)m.degree, m.off, 0LL, (size_t)n + 1, rocprim::plus<long long>(),
                                stream);
    if (e != hipSuccess) return e;
    if (numHits > 0)
        hipLaunchKernelGGL(neighbors_scatter_kernel, grid, block, 0, stream, skey, partner, ed, numHits, m.off, m.cursor,
                           m.partner, m.distance, m.position);
    return hipGetLastError();
}

}  // namespace edlib_amd
