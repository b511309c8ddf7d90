// self_components_core.hpp -- the connected components of a self batch's pairs within a level (edlibAmdBatchSelfComponents,
// DESIGN.md §4h "Components"): what one THREAD does.
//
// A lock-free union-find over parent[n], parent[i] = i at the start.  A thread owns one edge {i, j} and joins the two
// trees by hooking the LARGER root under the smaller with one compare-and-swap.  The invariant is parent[x] <= x, always:
//   * no cycles: a chain of parents descends strictly until it meets a root (parent[r] == r);
//   * a root is hooked once: the CAS expects parent[hi] == hi, and a vertex that has a smaller parent never gets itself
//     back, so a failed CAS returns a strictly smaller ancestor of hi and the retry starts below where it failed;
//   * the last root of a component is its smallest vertex, whatever the order of the edges: labels are canonical.
// No thread waits for another thread's store: every loop here ends by the thread's own progress (a parent chain that
// descends, a sum of two vertices that shrinks with every failed CAS).  There is no flag, no lock and no barrier.
//
// This header compiles for the device (self_components.hip: agent-scope HIP atomics) AND for the host
// (tests/self_components_host.cpp: the same code on __atomic builtins, edges split over std::threads, checked against a
// serial union-find: tests/test_self_components_model.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SC_FN __host__ __device__ __forceinline__
#else
#define SC_FN static inline __attribute__((always_inline))
#endif

namespace edlib_amd {
namespace self_components {

constexpr int kBlockThreads = 256;

// parent[] while edges are being hooked.  On the device a CU's L1 is not refreshed by other CUs' stores and a plain load
// may be hoisted out of a retry loop: every access is an agent-scope atomic (the loads and stores relaxed: they bypass
// L1; the CAS is performed where all CUs meet).
SC_FN int uf_load(const int* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
SC_FN void uf_store(int* p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}
// parent[*p] = desired if it is `expected`; returns what it was
SC_FN int uf_cas(int* p, int expected, int desired)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
    return expected;
}

// The root of x as this thread can see it, with path halving: x's parent becomes its grandparent on the way.
// Correctness does not depend on the halving, nor on how fresh a load is.  Every value parent[x] ever held is an ancestor
// of x (hooks only put a tree under a vertex of another, halving only skips a generation), so a stale load, or a halving
// store that puts back an older and wider parent over a newer one, still names an ancestor that is <= x: the chain
// descends to a vertex that WAS a root of x's component.  Whether it still is one is decided by the CAS of uf_union
// alone, and after the hook kernel by the kernel boundary.  A vertex that has a smaller parent is never stored its own
// index (the grandparent is <= the parent < x), so a root that was hooked stays hooked.
SC_FN int uf_find(int* parent, int x)
{
    for (;;) {
        const int p = uf_load(parent + x);
        if (p == x) return x;
        const int g = uf_load(parent + p);
        if (g == p) return p;
        uf_store(parent + x, g);
        x = g;
    }
}

// Joins the components of i and j.  Most edges of a dense family arrive when both ends hang under one root already: the
// two parents, loaded side by side, are ancestors of their vertices, so equal parents settle the edge with two loads;
// otherwise the join goes on from them (the trees of two ancestors are the trees of i and j).
SC_FN void uf_union(int* parent, int i, int j)
{
    int a = uf_load(parent + i), b = uf_load(parent + j);
    if (a == b) return;
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = uf_cas(parent + hi, hi, lo);
        if (old == hi) return;
        // hi was a root no more: old is a strictly smaller ancestor of it, and a + b shrinks
        a = old; b = lo;
    }
}

// After every hook is visible (the kernel boundary; the threads joined): the root by chasing only, plain loads
SC_FN int uf_chase(const int* parent, int x)
{
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    return x;
}

// Is a pair of reported distance d an edge at `level` (level < 0: every reported pair)?
SC_FN bool is_edge(int d, int level) { return d >= 0 && (level < 0 || d <= level); }

// Where pair (i, j), i < j, of n sequences sits in the condensed vector
SC_FN long long condensed_at(int n, int i, int j)
{
    return (long long)n * i - (long long)i * (i + 1) / 2 + (j - i - 1);
}

// The edge of one hit-list entry -- its row is the high half of its sorted key (i << 32) | j, which the list's finish
// leaves behind; the partner and the distance come from their planes -- / of one condensed cell
SC_FN void hook_hit(int* parent, const unsigned long long* skey, const int* partner, const int* ed, long long e, int level)
{
    if (is_edge(ed[e], level)) uf_union(parent, (int)(skey[e] >> 32), partner[e]);
}
SC_FN void hook_cell(int* parent, const int* cond, int n, int i, int j, int level)
{
    if (is_edge(cond[condensed_at(n, i, j)], level)) uf_union(parent, i, j);
}

}  // namespace self_components
}  // namespace edlib_amd
