// window_units.hip -- the queries and the unit list of a window batch prepared on the device (DESIGN.md §4i "Streamed
// units"): from the caller's offsets and unit arrays as they were uploaded, the rebased offsets of the query pool (of
// both strands where a unit names one), the units in the stable order (word group, window length, unit index) by
// rocPRIM's radix sort, a Peq slot for every pool entry some unit names (ascending entry inside its word group, by a
// stable 4-bit sort of the entries) and the per-unit arrays of the scan in sorted order.  No kernel here has an atomic:
// a mark is a plain store of the same byte, a group's bounds are binary searches of the sorted keys.  A translation unit
// of its own: rocPRIM's headers are most of its compile time.
#include "window_kernels.hpp"
#include "cross_kernels.hpp"

#include <rocprim/device/device_radix_sort.hpp>

namespace edlib_amd {

typedef uint32_t u32;

constexpr unsigned kLenBits = 17;                                 // window lengths 0..65,536 (kCrossMaxTarget)
constexpr unsigned kUnitKeyBits = kLenBits + 3;                   // and the word group - 1 (0..7) above them
constexpr unsigned kEntryKeyBits = 4;                             // word group - 1, or kWindowNoGroup
static_assert(kCrossMaxTarget < (1 << kLenBits), "a unit's key holds its window length in 17 bits");
static_assert(kCrossMaxQueryWords == 8 && kWindowNoGroup == 8, "a unit's key holds its word group in 3 bits");

__device__ __forceinline__ int words_of(long long m) { return m <= 32 ? 1 : (int)((m + 31) >> 5); }

// qoff[i] = offIn[i] - offIn[0] for i <= nq; both strands: entry 2 i starts at twice that, entry 2 i + 1 behind it, and
// the pool ends at qoff[2 nq] (the layout launch_strand_pool reads)
__global__ void __launch_bounds__(256)
window_query_offsets_kernel(const long long* __restrict__ offIn, int nq, int stranded, long long* __restrict__ qoff)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > nq) return;
    const long long base = offIn[0], o = offIn[i] - base;
    if (!stranded) { qoff[i] = o; return; }
    qoff[2 * (size_t)i] = 2 * o;
    if (i < nq) qoff[2 * (size_t)i + 1] = o + (offIn[i + 1] - base);
}

// key = ((words - 1) << 17) | unitLength, value = the unit, and its entry marked (every unit that names an entry stores
// the same 1: no atomic)
__global__ void __launch_bounds__(256)
window_unit_keys_kernel(WindowUnitsArgs a)
{
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= a.numUnits) return;
    const int q = a.unitQuery[u];
    const int e = a.unitStrand ? 2 * q + (int)a.unitStrand[u] : q;
    const int w = words_of(a.offIn[q + 1] - a.offIn[q]);
    a.ukey[u] = ((u32)(w - 1) << kLenBits) | (u32)a.unitLength[u];
    a.uval[u] = (u32)u;
    a.named[e] = 1;
}

// key of a pool entry: its word group - 1 where a unit names it, kWindowNoGroup (behind every group) where none does
__global__ void __launch_bounds__(256)
window_entry_keys_kernel(WindowUnitsArgs a)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.numEntries) return;
    const int q = a.unitStrand ? e >> 1 : e;
    a.ekey[e] = a.named[e] ? (u32)(words_of(a.offIn[q + 1] - a.offIn[q]) - 1) : (u32)kWindowNoGroup;
    a.eval[e] = (u32)e;
}

// bound[g], g <= kWindowNoGroup: the first sorted entry whose key is at least g -- entries of word group g + 1 are
// [bound[g], bound[g + 1])
__global__ void __launch_bounds__(64)
window_slot_bounds_kernel(const u32* __restrict__ ekeySorted, int numEntries, int* __restrict__ bound)
{
    const u32 g = threadIdx.x;
    if (g > (u32)kWindowNoGroup) return;
    int lo = 0, hi = numEntries;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ekeySorted[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    bound[g] = lo;
}

// the slot of every named entry: its place among the sorted entries of its word group
__global__ void __launch_bounds__(256)
window_entry_slots_kernel(const u32* __restrict__ ekeySorted, const int* __restrict__ entSorted, int numEntries,
                          const int* __restrict__ bound, int* __restrict__ slotOf)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= numEntries) return;
    const u32 g = ekeySorted[i];
    if (g < (u32)kWindowNoGroup) slotOf[entSorted[i]] = i - bound[g];
}

// per sorted position: the slot of the unit's entry, its start and its length (uperm is the sort's own output)
__global__ void __launch_bounds__(256)
window_unit_gather_kernel(WindowUnitsArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.numUnits) return;
    const int u = a.uperm[i];
    const int q = a.unitQuery[u];
    const int e = a.unitStrand ? 2 * q + (int)a.unitStrand[u] : q;
    a.uslot[i] = a.slotOf[e];
    a.ustart[i] = a.unitStart[u];
    a.ulen[i] = (int)(a.ukeySorted[i] & ((1u << kLenBits) - 1));
}

hipError_t window_units_tmp_bytes(int numUnits, int numEntries, size_t* bytes)
{
    size_t a = 0, b = 0;
    hipError_t e = hipSuccess;
    if (numUnits > 0)
        e = rocprim::radix_sort_pairs(nullptr, a, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr, (u32*)nullptr,
                                      (size_t)numUnits, 0u, kUnitKeyBits);
    if (e == hipSuccess && numEntries > 0)
        e = rocprim::radix_sort_pairs(nullptr, b, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr, (u32*)nullptr,
                                      (size_t)numEntries, 0u, kEntryKeyBits);
    *bytes = a > b ? a : b;
    return e;
}

hipError_t launch_window_query_offsets(const long long* offIn, int numQueries, bool stranded, long long* qoff,
                                       hipStream_t stream)
{
    hipLaunchKernelGGL(window_query_offsets_kernel, dim3((unsigned)(numQueries / 256 + 1)), dim3(256), 0, stream, offIn,
                       numQueries, stranded ? 1 : 0, qoff);
    return hipGetLastError();
}

hipError_t launch_window_units_prepare(const WindowUnitsArgs& a, void* tmp, size_t tmpBytes, hipStream_t stream)
{
    if (a.numUnits <= 0 || a.numEntries <= 0) return hipSuccess;
    const dim3 ugrid((unsigned)((a.numUnits + 255) / 256)), egrid((unsigned)((a.numEntries + 255) / 256));
    hipError_t e = hipMemsetAsync(a.named, 0, (size_t)a.numEntries, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(window_unit_keys_kernel, ugrid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(window_entry_keys_kernel, egrid, dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = tmpBytes;
    e = rocprim::radix_sort_pairs(tmp, bytes, (const u32*)a.ukey, a.ukeySorted, (const u32*)a.uval,
                                  reinterpret_cast<u32*>(a.uperm), (size_t)a.numUnits, 0u, kUnitKeyBits, stream);
    if (e != hipSuccess) return e;
    bytes = tmpBytes;
    e = rocprim::radix_sort_pairs(tmp, bytes, (const u32*)a.ekey, a.ekeySorted, (const u32*)a.eval,
                                  reinterpret_cast<u32*>(a.entSorted), (size_t)a.numEntries, 0u, kEntryKeyBits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(window_slot_bounds_kernel, dim3(1), dim3(64), 0, stream, (const u32*)a.ekeySorted, a.numEntries,
                       a.bound);
    hipLaunchKernelGGL(window_entry_slots_kernel, egrid, dim3(256), 0, stream, (const u32*)a.ekeySorted,
                       (const int*)a.entSorted, a.numEntries, (const int*)a.bound, a.slotOf);
    hipLaunchKernelGGL(window_unit_gather_kernel, ugrid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace edlib_amd
