// window_kernels.hip -- kernels of window batches (a query against a window of one resident target, DISTANCE only;
// DESIGN.md "Window batches").  A lane owns one unit and scans the whole height of its query (at most 8 words of 32 rows)
// over the columns of its window, which it reads from the one packed copy of the target; a wave is 64 units of one word
// group that are neighbours in window length, each with the Peq rows of its own query in LDS.
#include "window_kernels.hpp"
#include "cross_kernels.hpp"
#include "cross_column.hpp"

namespace edlib_amd {

typedef uint32_t u32;
typedef unsigned long long u64;

// ------------------------------------------------------------------- scan

// One wave per workgroup.  Staging: every lane copies the S x NWD Peq dwords of its query into its own column of the LDS
// slice [symbol][word][lane]; the lanes of a ds_read_b32 in the column loop then differ in symbol and so in address, but
// lane l always reads bank l % 32, alone in its 32-lane half: no conflict.  The only barrier is the one behind the staging.
template <int NWD, int S, int MODE>
__global__ void __launch_bounds__(64)
scan_windows_kernel(WindowScanArgs a)
{
    __shared__ u32 s_peq[S * NWD * 64];
    const int lane = threadIdx.x;
    const int u = blockIdx.x * 64 + lane;
    const bool live = u < a.numSorted;                  // padding lanes of the last wave do nothing
    int m = 0, n = 0, start = 0;
    if (live) {
        const int slot = a.uslot[u];
        m = a.qlen[slot]; n = a.ulen[u]; start = a.ustart[u];
        const u32* __restrict__ src = a.peq + (size_t)(slot >> 6) * (S * NWD * 64) + (slot & 63);
#pragma unroll 4
        for (int r = 0; r < S * NWD; ++r) s_peq[r * 64 + lane] = src[r * 64];
    }
    __syncthreads();
    if (!live) return;
    const int sh = (m - 1) & 31;
    int score = m, best = 0x7fffffff, cnt = 0, first = -1;
    if (m > 0 && n > 0 && !cross_nw_outside(MODE, a.kcfg, m, n)) {
        u32 Pv[NWD], Mv[NWD];
#pragma unroll
        for (int d = 0; d < NWD; ++d) { Pv[d] = ~0u; Mv[d] = 0u; }
        auto step = [&](u32 c, int j) {
            cross_column<NWD, MODE>(s_peq + c * (NWD * 64) + lane, 64, Pv, Mv, sh, score);
            if (MODE != 0) {
                if (score < best) { best = score; cnt = 1; first = j; }
                else if (score == best) ++cnt;
            }
        };
        // column j of the window is column start + j of the target: nibble (start + j) & 7 of dword (start + j) >> 3.
        // n > 0 and start + n <= targetLength (Create), so every dword read below holds a column of the target.
        const u32* __restrict__ tp = a.tpk + (start >> 3);
        u32 w = *tp >> (4 * (start & 7));               // the first dword, shifted to the window's first column
        const int have = 8 - (start & 7);
        const int head = have < n ? have : n;
        int j = 0;
        for (; j < head; ++j) { step(w & 15u, j); w >>= 4; }
        for (; j + 8 <= n; j += 8) {
            w = *++tp;
#pragma unroll
            for (int c = 0; c < 8; ++c) { step(w & 15u, j + c); w >>= 4; }
        }
        if (j < n) {
            w = *++tp;
            for (; j < n; ++j) { step(w & 15u, j); w >>= 4; }
        }
    }
    int ed, nloc, end;
    cross_cell_result(MODE, a.kcfg, m, n, MODE == 0 ? score : best, cnt, first, ed, nloc, end);
    const int at = a.uperm[u];
    a.ed[at] = ed; a.nloc[at] = nloc; a.end[at] = end;
}

template <int NWD, int S>
static hipError_t launch_scan_windows_ws(int mode, const WindowScanArgs& a, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.numSorted + 63) / 64));
    if (mode == 0) hipLaunchKernelGGL((scan_windows_kernel<NWD, S, 0>), grid, dim3(64), 0, stream, a);
    else if (mode == 1) hipLaunchKernelGGL((scan_windows_kernel<NWD, S, 1>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scan_windows_kernel<NWD, S, 2>), grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

template <int NWD>
static hipError_t launch_scan_windows_w(int syms, int mode, const WindowScanArgs& a, hipStream_t stream)
{
    if (syms == 4) return launch_scan_windows_ws<NWD, 4>(mode, a, stream);
    if (syms == 8) return launch_scan_windows_ws<NWD, 8>(mode, a, stream);
    return launch_scan_windows_ws<NWD, 16>(mode, a, stream);
}

hipError_t launch_scan_windows(int nwords, int syms, int mode, const WindowScanArgs& a, hipStream_t stream)
{
    if (a.numSorted == 0) return hipSuccess;
    if ((syms != 4 && syms != 8 && syms != 16) || mode < 0 || mode > 2 || a.numSorted < 0) return hipErrorInvalidValue;
    switch (nwords) {
    case 1: return launch_scan_windows_w<1>(syms, mode, a, stream);
    case 2: return launch_scan_windows_w<2>(syms, mode, a, stream);
    case 3: return launch_scan_windows_w<3>(syms, mode, a, stream);
    case 4: return launch_scan_windows_w<4>(syms, mode, a, stream);
    case 5: return launch_scan_windows_w<5>(syms, mode, a, stream);
    case 6: return launch_scan_windows_w<6>(syms, mode, a, stream);
    case 7: return launch_scan_windows_w<7>(syms, mode, a, stream);
    case 8: return launch_scan_windows_w<8>(syms, mode, a, stream);
    default: return hipErrorInvalidValue;
    }
}

// -------------------------------------------------------------- best unit

// pass 1: the smallest key (distance << 32) | unit per query; pass 2: the smallest key that is not the best.  Keys of
// different units differ, so the order of the atomics does not matter.  bkey = [best][nq], [second][nq], preset to ~0.
template <int PASS>
__global__ void __launch_bounds__(256)
window_best_kernel(const int* __restrict__ unitQuery, const int* __restrict__ ed, int numUnits, int numQueries,
                   u64* __restrict__ bkey)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= numUnits) return;
    const u64 key = cross_key(ed[i], (int)i);
    if (key == ~0ull) return;
    const int q = unitQuery[i];
    if (PASS == 1) atomicMin(bkey + q, key);
    else if (key != bkey[q]) atomicMin(bkey + numQueries + q, key);
}

__global__ void __launch_bounds__(256)
window_best_store_kernel(const u64* __restrict__ bkey, int numQueries, int* __restrict__ best)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= numQueries) return;
    const CrossBest2 r{bkey[q], bkey[numQueries + q]};
    best2_store(r, best, best + numQueries, best + 2 * (size_t)numQueries, q);
}

hipError_t launch_window_best(const int* unitQuery, const int* ed, int numUnits, int numQueries, u64* bkey, int* best,
                              hipStream_t stream)
{
    if (numQueries == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(bkey, 0xff, 2 * (size_t)numQueries * sizeof(u64), stream);
    if (e != hipSuccess) return e;
    if (numUnits > 0) {
        const dim3 grid((unsigned)(((long long)numUnits + 255) / 256));
        hipLaunchKernelGGL(window_best_kernel<1>, grid, dim3(256), 0, stream, unitQuery, ed, numUnits, numQueries, bkey);
        hipLaunchKernelGGL(window_best_kernel<2>, grid, dim3(256), 0, stream, unitQuery, ed, numUnits, numQueries, bkey);
    }
    hipLaunchKernelGGL(window_best_store_kernel, dim3((unsigned)((numQueries + 255) / 256)), dim3(256), 0, stream,
                       bkey, numQueries, best);
    return hipGetLastError();
}

}  // namespace edlib_amd
