// hit_list.hip -- the host side of the device hit list (hit_list.hpp): the buffers and their growth, the protocol behind
// the scans of a Run, and the finish steps the kinds of batch share -- rocPRIM's radix sort of (key, index), the offsets
// from the boundaries of the sorted keys, the gather of the planes into CSR order, the fetch as one pinned block.  The
// one translation unit that instantiates the sort: rocPRIM's headers are most of its compile time.
#include "hit_list.hpp"

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

namespace edlib_amd {

typedef uint32_t u32;
typedef unsigned long long u64;

// key bits the sort looks at: the low half and as many high bits as highValues - 1 needs
static unsigned key_end_bit(long long highValues)
{
    unsigned b = 0;
    while (b < 31 && (1LL << b) < highValues) ++b;
    return 32 + b;
}

__global__ void __launch_bounds__(256) hit_list_iota_kernel(u32* __restrict__ idx, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = (u32)i;
}

int HitListBuffers::size(size_t rows, long long minCap, hipStream_t stream)
{
    EDLIB_AMD_HIP(count.ensure(1));
    if (!pinned.p) EDLIB_AMD_HIP(pinned.alloc(2 * sizeof(u64)));
    rows_ = rows;
    if (rows > rowsCap_ || !res.p) {
        rowsCap_ = std::max(rows, rowsCap_);
        if (cap >= minCap) EDLIB_AMD_HIP(allocResult((size_t)cap));
    }
    return cap < minCap ? grow(minCap, stream) : 0;
}

// the list and its sort / CSR buffers for `cap` entries (what they held is gone)
int HitListBuffers::grow(long long newCap, hipStream_t stream)
{
    cap = 0;
    const size_t c = (size_t)newCap;
    size_t tmp = 0;
    hipError_t e = key.alloc(c);
    if (e == hipSuccess) e = val.alloc((size_t)planes_ * c);
    if (e == hipSuccess) e = idx.alloc(c);
    if (e == hipSuccess) e = skey.alloc(c);
    if (e == hipSuccess) e = sidx.alloc(c);
    if (e == hipSuccess) e = allocResult(c);
    if (e == hipSuccess && bytePlane_) e = byte.alloc(c);
    if (e == hipSuccess && bytePlane_) e = byteOut.alloc(c);
    if (e == hipSuccess && extraBytes_) e = extra.alloc((size_t)extraBytes_ * c);
    // (the most key bits a sort of this list may look at: the scratch does not grow with them)
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, tmp, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, c, 0u, 64u);
    if (e == hipSuccess) e = needScratch(tmp);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hit_list_iota_kernel, dim3((unsigned)((newCap + 255) / 256)), dim3(256), 0, stream, idx.p, newCap);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no room on the device for a hit list of %lld %s (%s)", prefix_, newCap, noun_, hipGetErrorString(e));
        return 1;
    }
    cap = newCap;
    return 0;
}

int HitListBuffers::afterScan(const HitRows& rows, int attempt, hipStream_t stream)
{
    u64* hc = reinterpret_cast<u64*>(pinned.p);
    EDLIB_AMD_HIP(hipMemcpyAsync(hc, count.p, sizeof *hc, hipMemcpyDeviceToHost, stream));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream));
    const long long appended = (long long)*hc, extra = (long long)rows.size(), total = appended + extra;
    if (total > cap) {
        if (total > (1LL << limitBits_) - 1) {
            set_error("%s: %lld %s, more than a hit list holds (2^%d - 1): lower k or split the batch", prefix_, total, noun_,
                      limitBits_);
            return 1;
        }
        if (attempt > 0) { set_error("%s: %lld %s after the list grew to %lld", prefix_, total, noun_, cap); return 1; }
        if (grow(total, stream)) return 1;
        if (appended > 0) {
            EDLIB_AMD_HIP(reset(stream));
            return kScanAgain;
        }
    }
    if (extra > 0) {
        const size_t c = (size_t)cap, x = (size_t)extra;
        EDLIB_AMD_HIP(hipMemcpyAsync(key.p + appended, rows.key.data(), x * sizeof(u64), hipMemcpyHostToDevice, stream));
        for (int f = 0; f < planes_; ++f)
            EDLIB_AMD_HIP(hipMemcpyAsync(val.p + f * c + appended, rows.val[f].data(), x * sizeof(int), hipMemcpyHostToDevice,
                                         stream));
        if (bytePlane_)
            EDLIB_AMD_HIP(hipMemcpyAsync(byte.p + appended, rows.byte.data(), x, hipMemcpyHostToDevice, stream));
    }
    n = total;
    return 0;
}

hipError_t HitListBuffers::sort(long long highValues, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned endBit = key_end_bit(highValues);
    size_t bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr,
                                             (u32*)nullptr, (size_t)n, 0u, endBit);
    if (e == hipSuccess) e = needScratch(bytes);
    if (e != hipSuccess) return e;
    bytes = tmp.n;
    // (a radix sort is stable: equal keys keep the order of the list)
    return rocprim::radix_sort_pairs(tmp.p, bytes, (const u64*)key.p, skey.p, (const u32*)idx.p, sidx.p, (size_t)n,
                                     0u, endBit, stream);
}

__global__ void __launch_bounds__(256)
hit_list_offsets_kernel(const u64* __restrict__ skey, long long n, int rows, long long* __restrict__ off)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > rows) return;
    const u64 want = (u64)(u32)r << 32;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skey[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    off[r] = lo;
}

hipError_t HitListBuffers::offsets(hipStream_t stream)
{
    const int rows = (int)rows_;
    hipLaunchKernelGGL(hit_list_offsets_kernel, dim3((unsigned)((rows + 1 + 255) / 256)), dim3(256), 0, stream, skey.p, n,
                       rows, off());
    return hipGetLastError();
}

template <int P>
__global__ void __launch_bounds__(256)
hit_list_gather_kernel(const u64* __restrict__ skey, const u32* __restrict__ sidx, const int* __restrict__ val, long long cap,
                       long long n, int* __restrict__ out, const uint8_t* __restrict__ byte, uint8_t* __restrict__ byteOut)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long j = sidx[i];
    out[i] = (int)(u32)skey[i];
#pragma unroll
    for (int f = 0; f < P; ++f) out[(f + 1) * n + i] = val[f * cap + j];
    if (byte) byteOut[i] = byte[j];
}

hipError_t HitListBuffers::gather(hipStream_t stream)
{
    outN = n;
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const uint8_t* bytes = bytePlane_ ? byte.p : nullptr;
    switch (planes_) {
#define CASE(P) case P: hipLaunchKernelGGL(hit_list_gather_kernel<P>, grid, block, 0, stream, skey.p, sidx.p, val.p, cap, \
                                           n, out(), bytes, byteOut.p); break;
        CASE(3) CASE(5)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int HitListBuffers::fetch(int planes, hipStream_t stream, const long long** off, const int** out)
{
    const size_t offBytes = (rows_ + 1) * sizeof(long long), listBytes = (size_t)planes * (size_t)outN * sizeof(int);
    if (!result.fetched) {
        EDLIB_AMD_HIP(result.fetch(res.p, offBytes + listBytes, stream));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream));
        result.fetched = true;
    }
    *off = reinterpret_cast<const long long*>(result.h.p);
    *out = reinterpret_cast<const int*>(result.h.p + offBytes);
    return 0;
}

}  // namespace edlib_amd
