// self_components.hip -- the connected components of a self batch's pairs within a level, labelled on the device
// (edlibAmdBatchSelfComponents, DESIGN.md §4h "Components"): init, hook (a thread per finished hit, or per condensed
// cell), flatten with the component counts, sizes, and -- where asked -- the members grouped by component with rocPRIM's
// stable radix sort of (label, index), head flags and an exclusive scan.  What a thread does with its edge is
// self_components_core.hpp.  Each step is a launch of its own: the kernel boundary publishes the hooks to the flatten.
#include "cross_kernels.hpp"
#include "self_components_core.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace edlib_amd {

namespace sc = self_components;
typedef uint32_t u32;

size_t SelfComponentsBuffers::ints(int n)
{
    return 10 * (size_t)n + 4;
}

SelfComponentsBuffers SelfComponentsBuffers::carve(int* base, int n)
{
    SelfComponentsBuffers b;
    const size_t m = (size_t)n;
    // what travels, back to back: label, componentSize, numComponents (and a pad), componentOffsets, members
    b.label = base; b.size = base + m; b.numComponents = base + 2 * m; b.offsets = base + 2 * m + 2;
    b.members = base + 3 * m + 3;
    b.parent = base + 4 * m + 4; b.count = b.parent + m; b.iota = b.count + m; b.slabel = b.iota + m;
    b.flag = b.slabel + m; b.rank = b.flag + m;
    return b;
}

__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_init_kernel(int n, int* __restrict__ parent, int* __restrict__ count, int* __restrict__ iota,
                            int* __restrict__ numComponents)
{
    const int i = blockIdx.x * sc::kBlockThreads + threadIdx.x;
    if (i == 0) *numComponents = 0;
    if (i >= n) return;
    parent[i] = i; count[i] = 0; iota[i] = i;
}

// a thread per finished hit: the row from the sorted key's high half, the partner and the distance from their planes
__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_hook_hits_kernel(const unsigned long long* __restrict__ skey, const int* __restrict__ partner,
                                 const int* __restrict__ ed, long long numHits, int level, int* parent)
{
    const long long e = (long long)blockIdx.x * sc::kBlockThreads + threadIdx.x;
    if (e < numHits) sc::hook_hit(parent, skey, partner, ed, e, level);
}

// a thread per condensed cell: block (x = row i, y = tile of 256 partners above i)
__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_hook_dense_kernel(const int* __restrict__ cond, int n, int level, int* parent)
{
    const int i = (int)blockIdx.x;
    const long long j = (long long)i + 1 + (long long)blockIdx.y * sc::kBlockThreads + threadIdx.x;
    if (j < n) sc::hook_cell(parent, cond, n, i, (int)j, level);
}

__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_flatten_kernel(const int* __restrict__ parent, int n, int* __restrict__ label, int* __restrict__ count)
{
    const int i = blockIdx.x * sc::kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const int r = sc::uf_chase(parent, i);
    label[i] = r;
    atomicAdd(count + r, 1);
}

__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_sizes_kernel(const int* __restrict__ label, const int* __restrict__ count, int n, int* __restrict__ size,
                             int* __restrict__ numComponents)
{
    __shared__ int roots;
    if (threadIdx.x == 0) roots = 0;
    __syncthreads();
    const int i = blockIdx.x * sc::kBlockThreads + threadIdx.x;
    if (i < n) {
        const int r = label[i];
        size[i] = count[r];
        if (r == i) atomicAdd(&roots, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && roots) atomicAdd(numComponents, roots);
}

// members: sorted by (label, index), position p starts a component where its label differs from the one before
__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_heads_kernel(const int* __restrict__ slabel, int n, int* __restrict__ flag)
{
    const int p = blockIdx.x * sc::kBlockThreads + threadIdx.x;
    if (p < n) flag[p] = p == 0 || slabel[p] != slabel[p - 1];
}

// rank[p]: components that start before p.  offsets[c] = the start of component c, offsets[numComponents] = n
__global__ void __launch_bounds__(sc::kBlockThreads)
self_components_offsets_kernel(const int* __restrict__ flag, const int* __restrict__ rank, int n, int* __restrict__ offsets)
{
    const int p = blockIdx.x * sc::kBlockThreads + threadIdx.x;
    if (p >= n) return;
    if (flag[p]) offsets[rank[p]] = p;
    if (p == n - 1) offsets[rank[p] + flag[p]] = n;
}

static unsigned label_bits(int n)
{
    unsigned b = 1;
    while (b < 31 && (1LL << b) < n) ++b;
    return b;
}

hipError_t self_components_scratch(int n, size_t* bytes)
{
    size_t sortBytes = 0, scanBytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sortBytes, (const u32*)nullptr, (u32*)nullptr, (const int*)nullptr,
                                             (int*)nullptr, (size_t)n, 0u, label_bits(n));
    if (e == hipSuccess)
        e = rocprim::exclusive_scan(nullptr, scanBytes, (const int*)nullptr, (int*)nullptr, 0, (size_t)n, rocprim::plus<int>());
    *bytes = sortBytes > scanBytes ? sortBytes : scanBytes;
    return e;
}

hipError_t launch_self_components(const SelfComponentsBuffers& b, int n, const unsigned long long* skey, const int* partner,
                                  const int* ed, long long numHits, const int* cond, int level, bool members,
                                  void* scratch, size_t scratchBytes, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const dim3 block(sc::kBlockThreads), rows((unsigned)((n + sc::kBlockThreads - 1) / sc::kBlockThreads));
    hipLaunchKernelGGL(self_components_init_kernel, rows, block, 0, stream, n, b.parent, b.count, b.iota, b.numComponents);
    if (cond) {
        if (rows.x > 65535u) return hipErrorInvalidValue;             // (a condensed vector of 2^47 ints)
        if (n > 1)
            hipLaunchKernelGGL(self_components_hook_dense_kernel, dim3((unsigned)(n - 1), rows.x), block, 0, stream, cond, n,
                               level, b.parent);
    } else if (numHits > 0)
        hipLaunchKernelGGL(self_components_hook_hits_kernel,
                           dim3((unsigned)((numHits + sc::kBlockThreads - 1) / sc::kBlockThreads)), block, 0, stream, skey,
                           partner, ed, numHits, level, b.parent);
    hipLaunchKernelGGL(self_components_flatten_kernel, rows, block, 0, stream, b.parent, n, b.label, b.count);
    hipLaunchKernelGGL(self_components_sizes_kernel, rows, block, 0, stream, b.label, b.count, n, b.size, b.numComponents);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !members) return e;
    // (a radix sort is stable: the members of a component stay in ascending order)
    size_t bytes = scratchBytes;
    e = rocprim::radix_sort_pairs(scratch, bytes, (const u32*)b.label, (u32*)b.slabel, (const int*)b.iota, b.members,
                                  (size_t)n, 0u, label_bits(n), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(self_components_heads_kernel, rows, block, 0, stream, b.slabel, n, b.flag);
    bytes = scratchBytes;
    e = rocprim::exclusive_scan(scratch, bytes, (const int*)b.flag, b.rank, 0, (size_t)n, rocprim::plus<int>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(self_components_offsets_kernel, rows, block, 0, stream, b.flag, b.rank, n, b.offsets);
    return hipGetLastError();
}

}  // namespace edlib_amd
