// reads_hits.hip -- hit-list read batches: every maximal run of target columns where a read scores <= k.
//   * the HITS instantiations of the banded HW scan (reads_scan.hpp) and of the seed + verify kernel (reads_seed.hpp): the
//     threshold stays at min(k, m), each lane follows its open run in registers and appends closed runs to one device list;
//   * the read batch's own part of the finish: the list's keys go from slots to units before the list's sort (hit_list.hpp)
//     orders them by (unit, firstEnd), runs that meet at a segment boundary are stitched, and the offsets per unit come from
//     the stitched list.
// A translation unit of its own: the other scans carry none of it.
#include "reads_seed.hpp"

#include <rocprim/device/device_scan.hpp>

namespace edlib_amd {

// ------------------------------------------------------------------ the scans

template <int S>
static hipError_t launch_scan_reads_hits_s(int nwords, const ReadScanArgs& a, hipStream_t stream)
{
    dim3 grid((a.nlanes + 63) / 64, a.numSegments), block(64);
    switch (nwords) {
#define CASE(N) case N: EDLIB_AMD_CHECK_STATIC_LDS((scan_reads_banded_kernel<N, S, false, true>), N * S * 256); \
                        hipLaunchKernelGGL((scan_reads_banded_kernel<N, S, false, true>), grid, block, 0, stream, a); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scan_reads_hits(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream)
{
    if (a.nlanes == 0) return hipSuccess;
    if (!a.hits.key || !a.hits.val || !a.hits.count || a.hits.cap <= 0) return hipErrorInvalidValue;
    switch (syms) {
        case 4: return launch_scan_reads_hits_s<4>(nwords, a, stream);
        case 8: return launch_scan_reads_hits_s<8>(nwords, a, stream);
        case 16: return launch_scan_reads_hits_s<16>(nwords, a, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_seed_verify_hits(int nwords, const SeedArgs& a, hipStream_t stream)
{
    if (a.nslots == 0) return hipSuccess;
    if (!a.hits.key || !a.hits.val || !a.hits.count || a.hits.cap <= 0) return hipErrorInvalidValue;
    const dim3 grid(a.nslots / 64), block(64);
    switch (nwords) {
#define CASE(N) case N: hipLaunchKernelGGL((seed_verify_kernel<N, true>), grid, block, 0, stream, a); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ the finish

// slot keys -> unit keys; a padding slot (it scans a one-symbol read that nobody asked for) sorts behind every unit
__global__ void __launch_bounds__(256)
read_hits_keys_kernel(u64* __restrict__ key, long long n, const int* __restrict__ slotUnit, int numUnits)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    const int u = slotUnit[(u32)(k >> 32)];
    key[i] = ((u64)(u32)(u < 0 ? numUnits : u) << 32) | (u32)k;
}

// head[i] = 1: sorted run i starts a hit (it is no padding and does not continue the run before it)
__global__ void __launch_bounds__(256)
read_hits_heads_kernel(const u64* __restrict__ skey, const u32* __restrict__ sidx, const int* __restrict__ val, long long n,
                       int numUnits, u32* __restrict__ head)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = skey[i];
    bool h = (int)(k >> 32) < numUnits;
    if (h && i > 0) {
        const u64 p = skey[i - 1];
        if ((p >> 32) == (k >> 32) && val[sidx[i - 1]] + 1 == (int)(u32)k) h = false;       // lastEnd + 1 == firstEnd
    }
    head[i] = h ? 1u : 0u;
}

__global__ void read_hits_total_kernel(const u32* __restrict__ head, const u32* __restrict__ at, long long n, long long* total)
{
    *total = (long long)at[n - 1] + head[n - 1];
}

// The thread of a head walks the runs that continue it (a run spanning s segments has s pieces): the distance is the least,
// endLocation the first column holding it (pieces ascend), numLocations the sum over the pieces whose least equals it.
__global__ void __launch_bounds__(256)
read_hits_stitch_kernel(const u64* __restrict__ skey, const u32* __restrict__ sidx, const int* __restrict__ val, long long cap,
                        long long n, int numUnits, const u32* __restrict__ head, const u32* __restrict__ at,
                        const long long* __restrict__ total, int* __restrict__ out, int* __restrict__ outUnit)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !head[i]) return;
    const long long H = *total;
    long long j = sidx[i];
    int last = val[j], ed = val[cap + j], pos = val[2 * cap + j], cnt = val[3 * cap + j];
    for (long long t = i + 1; t < n && !head[t] && (int)(skey[t] >> 32) < numUnits; ++t) {
        j = sidx[t];
        const int ed2 = val[cap + j];
        if (ed2 < ed) { ed = ed2; pos = val[2 * cap + j]; cnt = val[3 * cap + j]; }
        else if (ed2 == ed) cnt += val[3 * cap + j];
        last = val[j];
    }
    const long long o = at[i];
    out[o] = (int)(u32)skey[i]; out[H + o] = last; out[2 * H + o] = ed; out[3 * H + o] = pos; out[4 * H + o] = cnt;
    outUnit[o] = (int)(skey[i] >> 32);
}

// unitOffsets[u] = first hit of unit u or later (u = numUnits: all of them)
__global__ void __launch_bounds__(256)
read_hits_offsets_kernel(const int* __restrict__ outUnit, const long long* __restrict__ total, int numUnits,
                         long long* __restrict__ uoff)
{
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u > numUnits) return;
    long long lo = 0, hi = *total;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (outUnit[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    uoff[u] = lo;
}

hipError_t launch_read_hits_finish(HitListBuffers& hl, const int* slotUnit, int numUnits, long long* total, hipStream_t stream)
{
    const long long n = hl.n, cap = hl.cap;
    if (n <= 0 || n > 0x7fffffffLL) return hipErrorInvalidValue;
    u32* head = reinterpret_cast<u32*>(hl.extra.p);
    u32* at = head + cap;
    int* outUnit = reinterpret_cast<int*>(at + cap);
    size_t scanBytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scanBytes, (const u32*)nullptr, (u32*)nullptr, 0u, (size_t)n, rocprim::plus<u32>());
    if (e == hipSuccess) e = hl.needScratch(scanBytes);
    if (e != hipSuccess) return e;
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(read_hits_keys_kernel, dim3(nb), dim3(256), 0, stream, hl.key.p, n, slotUnit, numUnits);
    e = hl.sort((long long)numUnits + 1, stream);              // (the padding's key is numUnits)
    if (e != hipSuccess) return e;
    const u64* skey = hl.skey.p;
    const u32* sidx = hl.sidx.p;
    hipLaunchKernelGGL(read_hits_heads_kernel, dim3(nb), dim3(256), 0, stream, skey, sidx, hl.val.p, n, numUnits, head);
    scanBytes = hl.tmp.n;
    e = rocprim::exclusive_scan(hl.tmp.p, scanBytes, (const u32*)head, at, 0u, (size_t)n, rocprim::plus<u32>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(read_hits_total_kernel, dim3(1), dim3(1), 0, stream, head, at, n, total);
    hipLaunchKernelGGL(read_hits_stitch_kernel, dim3(nb), dim3(256), 0, stream, skey, sidx, hl.val.p, cap, n, numUnits, head, at,
                       total, hl.out(), outUnit);
    hipLaunchKernelGGL(read_hits_offsets_kernel, dim3((unsigned)((numUnits + 1 + 255) / 256)), dim3(256), 0, stream,
                       outUnit, total, numUnits, hl.off());
    return hipGetLastError();
}

}  // namespace edlib_amd
