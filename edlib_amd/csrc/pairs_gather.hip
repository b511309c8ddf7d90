// pairs_gather.hip -- the pools of a flat pair set gathered on the device from a window batch's resident query pool and
// 4-bit target pack (edlibAmdBatchPairsSetWindows; DESIGN.md §4b "Pairs from a window batch"), or from a read batch's
// query pool and raw target (edlibAmdBatchPairsSetSharedWindows; "Pairs from a read batch"), or from a cross or self
// batch's query pool and its pack of many targets (edlibAmdBatchPairsSetCells; "Pairs from a cross batch": a plan kernel
// writes every pair's 64-bit nibble position in that pack first).  Pure data movement: a
// thread owns 16 aligned destination bytes (pairs_gather_core.hpp) and a wave stores 1 KiB of consecutive bytes per
// instruction.  A block first narrows the offsets to the pairs its 4 KiB touch -- every wave searches the same two
// positions, 64 probes a step -- so that a thread's own binary search runs over a handful of pairs.
#include "pairs_gather.hpp"
#include "pairs_gather_core.hpp"
#include "strands.hpp"

namespace edlib_amd {

using namespace pairs_gather;

struct IdToByte { uint8_t b[16]; };

// The largest p in [lo, hi] with off[p] <= pos, by a whole wave (every lane with the same arguments): a lane a probe, the
// ballot counts the probes at or below pos
__device__ __forceinline__ int find_pair_wave(const long long* __restrict__ off, int lo, int hi, long long pos)
{
    const int lane = threadIdx.x & 63;
    while (lo < hi) {
        const long long at = probe_at(lo, hi, lane);
        const bool below = at <= hi && off[at] <= pos;
        narrow(lo, hi, __popcll(__ballot(below)));
    }
    return lo;
}

// the pairs [lo, hi] that hold the bytes of this block (called by whole waves)
__device__ __forceinline__ void block_pairs(const long long* __restrict__ off, int n, long long total, int& lo, int& hi)
{
    lo = find_pair_wave(off, 0, n - 1, block_first(total, blockIdx.x));
    hi = find_pair_wave(off, lo, block_far(lo, n), block_last(total, blockIdx.x));
}

// the run of thread `d0 / 16`: 16 bytes where the pool (total + 16 bytes) has them, the pool's last bytes one by one
__device__ __forceinline__ void store_run(uint8_t* __restrict__ pool, long long d0, long long total, const Run& r)
{
    const long long left = total + 16 - d0;
    if (left >= kRun) {
        uint4 v;
        v.x = (u32)r.w[0]; v.y = (u32)(r.w[0] >> 32); v.z = (u32)r.w[1]; v.w = (u32)(r.w[1] >> 32);
        *reinterpret_cast<uint4*>(pool + d0) = v;
    } else {
        for (int j = 0; j < (int)left; ++j) pool[d0 + j] = (uint8_t)(r.w[j >> 3] >> (8 * (j & 7)));
    }
}

__global__ void __launch_bounds__(kBlockThreads)
gather_targets_kernel(const long long* __restrict__ toff, int n, long long total, TargetSource src, IdToByte ids,
                      uint8_t* __restrict__ tpool)
{
    __shared__ uint16_t s_tab2[256];
    s_tab2[threadIdx.x] = (uint16_t)(ids.b[threadIdx.x & 15] | ids.b[threadIdx.x >> 4] << 8);
    __syncthreads();
    int lo, hi;
    block_pairs(toff, n, total, lo, hi);                         // (every lane of every wave: before any of them leaves)
    const long long d0 = ((long long)blockIdx.x * kBlockThreads + threadIdx.x) * kRun;
    if (d0 >= total + 16) return;
    Run r; r.w[0] = 0; r.w[1] = 0;
    if (d0 < total) {
        r = target_run(d0, total, find_pair(toff, lo, hi, d0), toff, src, s_tab2);
    }
    store_run(tpool, d0, total, r);
}

// store_run with the run's two words named, not indexed: the run stays in registers (an indexed `r.w[j >> 3]` makes the
// compiler keep every thread's run in LDS, 4 KiB a block, on the full-store path too)
__device__ __forceinline__ void store_run_words(uint8_t* __restrict__ pool, long long d0, long long total, u64 w0, u64 w1)
{
    const long long left = total + 16 - d0;
    if (left >= kRun) {
        uint4 v;
        v.x = (u32)w0; v.y = (u32)(w0 >> 32); v.z = (u32)w1; v.w = (u32)(w1 >> 32);
        *reinterpret_cast<uint4*>(pool + d0) = v;
    } else {
        for (int j = 0; j < (int)left; ++j) pool[d0 + j] = (uint8_t)((j < 8 ? w0 : w1) >> (8 * (j & 7)));
    }
}

// the same from a target that is resident as bytes (a read batch's target pool): no table, a run inside one pair is five
// dwords funnel-shifted
__global__ void __launch_bounds__(kBlockThreads)
gather_targets_bytes_kernel(const long long* __restrict__ toff, int n, long long total, TargetBytesSource src,
                            uint8_t* __restrict__ tpool)
{
    int lo, hi;
    block_pairs(toff, n, total, lo, hi);                         // (every lane of every wave: before any of them leaves)
    const long long d0 = ((long long)blockIdx.x * kBlockThreads + threadIdx.x) * kRun;
    if (d0 >= total + 16) return;
    Run r; r.w[0] = 0; r.w[1] = 0;
    if (d0 < total) {
        r = target_run_bytes(d0, total, find_pair(toff, lo, hi, d0), toff, src);
    }
    store_run_words(tpool, d0, total, r.w[0], r.w[1]);
}

__global__ void __launch_bounds__(kBlockThreads)
gather_queries_kernel(const long long* __restrict__ qoff, int n, long long total, QuerySource src, uint8_t* __restrict__ qpool)
{
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = complement_byte((uint8_t)threadIdx.x);
    __syncthreads();
    int lo, hi;
    block_pairs(qoff, n, total, lo, hi);                         // (every lane of every wave: before any of them leaves)
    const long long d0 = ((long long)blockIdx.x * kBlockThreads + threadIdx.x) * kRun;
    if (d0 >= total + 16) return;
    Run r; r.w[0] = 0; r.w[1] = 0;
    if (d0 < total) {
        r = query_run(d0, total, find_pair(qoff, lo, hi, d0), qoff, src, s_comp);
    }
    store_run(qpool, d0, total, r);
}

// ---- a cross or self batch's pack: many targets back to back (edlibAmdBatchPairsSetCells; "Pairs from a cross batch")

// place[tperm[i]] = i: where every target lies in the pack's order (place was filled with -1)
__global__ void __launch_bounds__(kBlockThreads)
pack_places_kernel(const int* __restrict__ tperm, int numSorted, int* __restrict__ place)
{
    const int i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i < numSorted) place[tperm[i]] = i;
}

// the plan: one thread a pair, the 64-bit nibble position of its window's first column (pairStart null: column 0)
__global__ void __launch_bounds__(kBlockThreads)
plan_cells_kernel(const int* __restrict__ pairTarget, const int* __restrict__ pairStart, const int* __restrict__ place,
                  const long long* __restrict__ tdw, int n, long long* __restrict__ base)
{
    const int p = blockIdx.x * kBlockThreads + threadIdx.x;
    if (p < n) base[p] = cell_base(place, tdw, pairTarget[p], pairStart ? pairStart[p] : 0);
}

// gather_targets_kernel over that pack: the window of pair p starts at nibble src.pairBase[p]
__global__ void __launch_bounds__(kBlockThreads)
gather_targets_cells_kernel(const long long* __restrict__ toff, int n, long long total, TargetCellsSource src, IdToByte ids,
                            uint8_t* __restrict__ tpool)
{
    __shared__ uint16_t s_tab2[256];
    s_tab2[threadIdx.x] = (uint16_t)(ids.b[threadIdx.x & 15] | ids.b[threadIdx.x >> 4] << 8);
    __syncthreads();
    int lo, hi;
    block_pairs(toff, n, total, lo, hi);                         // (every lane of every wave: before any of them leaves)
    const long long d0 = ((long long)blockIdx.x * kBlockThreads + threadIdx.x) * kRun;
    if (d0 >= total + 16) return;
    Run r; r.w[0] = 0; r.w[1] = 0;
    if (d0 < total) {
        r = target_run_cells(d0, total, find_pair(toff, lo, hi, d0), toff, src, s_tab2);
    }
    store_run_words(tpool, d0, total, r.w[0], r.w[1]);
}

static unsigned gather_blocks(long long bytes) { return (unsigned)((bytes + 16 + kBlockBytes - 1) / kBlockBytes); }

hipError_t launch_pack_places(const int* tperm, int numSorted, int* place, int numTargets, hipStream_t stream)
{
    if (numTargets < 1 || numSorted < 0 || numSorted > numTargets || !place || (numSorted > 0 && !tperm)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(place, 0xff, (size_t)numTargets * sizeof(int), stream);
    if (e != hipSuccess || numSorted == 0) return e;
    hipLaunchKernelGGL(pack_places_kernel, dim3((unsigned)((numSorted + kBlockThreads - 1) / kBlockThreads)), dim3(kBlockThreads),
                       0, stream, tperm, numSorted, place);
    return hipGetLastError();
}

hipError_t launch_pairs_gather_cells(const CellSource& c, const CellsGatherArgs& ca, hipStream_t stream)
{
    const PairsGatherArgs& a = ca.pools;
    if (a.numPairs < 1 || a.qbytes < 1 || a.tbytes < 1) return hipErrorInvalidValue;
    if (!c.d_qpool || !c.d_qoff || !c.d_pack || !c.d_tdw || !c.d_place || !ca.pairTarget || !ca.pairBase || c.packDwords < 1)
        return hipErrorInvalidValue;
    // the wide accesses: dwords of the sources, 128-bit stores into the pools, 64-bit bases
    if ((reinterpret_cast<uintptr_t>(c.d_qpool) & 3) || (reinterpret_cast<uintptr_t>(c.d_pack) & 3) ||
        (reinterpret_cast<uintptr_t>(ca.pairBase) & 7) ||
        (reinterpret_cast<uintptr_t>(a.qpool) & 15) || (reinterpret_cast<uintptr_t>(a.tpool) & 15)) return hipErrorInvalidValue;
    if ((a.qbytes + 16 + kBlockBytes - 1) / kBlockBytes > 0x7fffffffLL || (a.tbytes + 16 + kBlockBytes - 1) / kBlockBytes > 0x7fffffffLL)
        return hipErrorInvalidValue;

    hipLaunchKernelGGL(plan_cells_kernel, dim3((unsigned)((a.numPairs + kBlockThreads - 1) / kBlockThreads)), dim3(kBlockThreads),
                       0, stream, ca.pairTarget, a.pairStart, c.d_place, c.d_tdw, a.numPairs, ca.pairBase);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    TargetCellsSource ts{};
    ts.pack = c.d_pack; ts.ndw = c.packDwords; ts.pairBase = ca.pairBase;
    IdToByte ids;
    for (int i = 0; i < 16; ++i) ids.b[i] = c.idToByte[i];
    hipLaunchKernelGGL(gather_targets_cells_kernel, dim3(gather_blocks(a.tbytes)), dim3(kBlockThreads), 0, stream,
                       a.toff, a.numPairs, a.tbytes, ts, ids, a.tpool);
    e = hipGetLastError();
    if (e != hipSuccess) return e;

    QuerySource qs{};
    qs.pool = reinterpret_cast<const u32*>(c.d_qpool); qs.ndw = (long long)(c.qpoolBytes / 4);
    qs.off = c.d_qoff; qs.stranded = c.stranded ? 1 : 0;
    qs.pairQuery = a.pairQuery; qs.pairStrand = a.pairStrand;
    hipLaunchKernelGGL(gather_queries_kernel, dim3(gather_blocks(a.qbytes)), dim3(kBlockThreads), 0, stream,
                       a.qoff, a.numPairs, a.qbytes, qs, a.qpool);
    return hipGetLastError();
}

hipError_t launch_pairs_gather(const WindowSource& w, const PairsGatherArgs& a, hipStream_t stream)
{
    static_assert(kBlockThreads == 256, "a block fills its 256-entry tables with one entry per thread");
    static_assert(kProbes == 64, "a probe per lane of a wave");
    if (a.numPairs < 1 || a.qbytes < 1 || a.tbytes < 1) return hipErrorInvalidValue;
    // the wide accesses: dwords of the sources, 128-bit stores into the pools
    if ((reinterpret_cast<uintptr_t>(w.d_qpool) & 3) || (reinterpret_cast<uintptr_t>(w.d_pack) & 3) ||
        (reinterpret_cast<uintptr_t>(w.d_tbytes) & 3) ||
        (reinterpret_cast<uintptr_t>(a.qpool) & 15) || (reinterpret_cast<uintptr_t>(a.tpool) & 15)) return hipErrorInvalidValue;
    // (the target: a pack or bytes, one of the two; every window lies inside what is allocated, whose dwords bound the loads)
    if ((w.d_pack != nullptr) == (w.d_tbytes != nullptr)) return hipErrorInvalidValue;
    if (w.d_tbytes && (long long)(w.tbytesAlloc / 4) * 4 < (long long)w.targetLength) return hipErrorInvalidValue;
    const auto blocks = [](long long bytes) { return (unsigned)((bytes + 16 + kBlockBytes - 1) / kBlockBytes); };
    if ((a.qbytes + 16 + kBlockBytes - 1) / kBlockBytes > 0x7fffffffLL || (a.tbytes + 16 + kBlockBytes - 1) / kBlockBytes > 0x7fffffffLL)
        return hipErrorInvalidValue;

    if (w.d_tbytes) {
        TargetBytesSource tb{};
        tb.bytes = reinterpret_cast<const u32*>(w.d_tbytes); tb.ndw = (long long)(w.tbytesAlloc / 4); tb.pairStart = a.pairStart;
        hipLaunchKernelGGL(gather_targets_bytes_kernel, dim3(blocks(a.tbytes)), dim3(kBlockThreads), 0, stream,
                           a.toff, a.numPairs, a.tbytes, tb, a.tpool);
    } else {
        TargetSource ts{};
        ts.pack = w.d_pack; ts.ndw = w.packDwords; ts.pairStart = a.pairStart;
        IdToByte ids;
        for (int i = 0; i < 16; ++i) ids.b[i] = w.idToByte[i];
        hipLaunchKernelGGL(gather_targets_kernel, dim3(blocks(a.tbytes)), dim3(kBlockThreads), 0, stream,
                           a.toff, a.numPairs, a.tbytes, ts, ids, a.tpool);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    QuerySource qs{};
    qs.pool = reinterpret_cast<const u32*>(w.d_qpool); qs.ndw = (long long)(w.qpoolBytes / 4);
    qs.off = w.d_qoff; qs.stranded = w.stranded ? 1 : 0;
    qs.pairQuery = a.pairQuery; qs.pairStrand = a.pairStrand;
    hipLaunchKernelGGL(gather_queries_kernel, dim3(blocks(a.qbytes)), dim3(kBlockThreads), 0, stream,
                       a.qoff, a.numPairs, a.qbytes, qs, a.qpool);
    return hipGetLastError();
}

}  // namespace edlib_amd
