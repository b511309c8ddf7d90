// reads_seed.hip -- exact k-mer seed filter of the reads-per-lane path: the first pass of an HW group of
// reads up to 256 bases against a shared target of at most four symbols, in place of the banded scan over every column.
//
// A read of m symbols is cut into p = k + 1 consecutive pieces (lengths floor(m / p) or one more).  An alignment with <= k
// edits leaves one piece without an edit (pigeonhole), so that piece occurs exactly in the target, and the alignment lies in
// the window [delta - k, delta + m - 1 + k] of the diagonal delta = P - o of that occurrence.  An HW scan restarted at the
// window's first column computes D' >= D for every column of the window, with equality wherever D <= k (the restart rule of
// DESIGN.md §1).  So: look every piece up exactly, merge the windows of a read, scan them with the whole read, and the least
// D' over the windows with the columns attaining it are the reads path's result whenever that least value is <= k.
// tests/seed_model.py is the same argument in numpy, checked against the textbook DP.
//
//   * the index: direct-address buckets on the first kSeedQ = 12 symbols of every target position (4^12 + 1 offsets,
//     T positions), built from the 2-bit packed target by a count kernel, rocPRIM's exclusive scan and a fill kernel;
//   * the seed + verify kernel: a lane per slot, a wave 64 consecutive slots (kernel A's layout).  The lane's Peq rows
//     (g.d_peq, [readBlock][4][NWD][64]) are its read: the 2-bit code of a query symbol is which row has its bit, a symbol
//     in no row (a byte the target lacks) makes its piece impossible.  Diagonals go into a sorted, duplicate-free list in
//     LDS; windows are merged and verified with the column of scan_reads_kernel, the target symbol of a lane's column
//     gathered from the packed target and its Eq row picked per lane from the four rows.
//   * hand-back: a read whose lookup is not cheap (a bucket of more than kSeedBucketCap positions, more than
//     kSeedMaxDiag distinct diagonals, a merged window longer than kSeedMaxWindow columns, a piece shorter than kSeedQ) is
//     listed; the host scans the list with the banded kernel over the whole target at the same threshold.
#include "reads_kernels.hpp"
#include "reads_scan.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace edlib_amd {

typedef unsigned long long u64;

// 2n bits (n <= 16 symbols) of a 2-bit stream starting at symbol x: the stream holds 16 symbols per dword, LSB first
__device__ __forceinline__ u32 stream_bits(u32 lo, u32 hi, u32 x) { return (u32)((((u64)hi << 32) | lo) >> (2 * (x & 15))); }

// 16 bits -> the even bits of a dword (bit i -> bit 2i)
__device__ __forceinline__ u32 spread16(u32 x)
{
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}

// a[i] for a lane-varying i without indexing the register array (dynamic indexing would put it in scratch); 0 past the end
template <int N>
__device__ __forceinline__ u32 pick(const u32 (&a)[N], int i)
{
    u32 r = 0;
#pragma unroll
    for (int d = 0; d < N; ++d) r = (i == d) ? a[d] : r;
    return r;
}

// ------------------------------------------------------------------ the index

__global__ void __launch_bounds__(256)
seed_count_kernel(const u32* __restrict__ tpk, int npos, u32* __restrict__ cnt)
{
    const int P = blockIdx.x * blockDim.x + threadIdx.x;
    if (P >= npos) return;
    const u32 key = stream_bits(tpk[P >> 4], tpk[(P >> 4) + 1], (u32)P) & ((1u << (2 * kSeedQ)) - 1u);
    atomicAdd(&cnt[key], 1u);
}

// cnt counts down to zero again, so the next run's count starts from a zeroed table as well
__global__ void __launch_bounds__(256)
seed_fill_kernel(const u32* __restrict__ tpk, int npos, const u32* __restrict__ off, u32* __restrict__ cnt,
                 u32* __restrict__ pos)
{
    const int P = blockIdx.x * blockDim.x + threadIdx.x;
    if (P >= npos) return;
    const u32 key = stream_bits(tpk[P >> 4], tpk[(P >> 4) + 1], (u32)P) & ((1u << (2 * kSeedQ)) - 1u);
    pos[off[key] + atomicSub(&cnt[key], 1u) - 1u] = (u32)P;
}

hipError_t seed_index_scratch_bytes(size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const u32*)nullptr, (u32*)nullptr, 0u, kSeedBuckets + 1,
                                   rocprim::plus<u32>());
}

hipError_t launch_build_seed_index(const u32* tpk, int T, u32* cnt, u32* off, u32* pos, void* tmp, size_t tmpBytes,
                                   hipStream_t stream)
{
    const int npos = T - kSeedQ + 1;                      // positions with a whole key
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)(kSeedBuckets + 1) * sizeof(u32), stream);
    if (e != hipSuccess) return e;
    if (npos > 0) {
        hipLaunchKernelGGL(seed_count_kernel, dim3((npos + 255) / 256), dim3(256), 0, stream, tpk, npos, cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    size_t bytes = tmpBytes;
    e = rocprim::exclusive_scan(tmp, bytes, cnt, off, 0u, kSeedBuckets + 1, rocprim::plus<u32>(), stream);
    if (e != hipSuccess || npos <= 0) return e;
    hipLaunchKernelGGL(seed_fill_kernel, dim3((npos + 255) / 256), dim3(256), 0, stream, tpk, npos, off, cnt, pos);
    return hipGetLastError();
}

// ------------------------------------------------------------ seed + verify

template <int NWD>
__global__ void __launch_bounds__(64)
seed_verify_kernel(const SeedArgs a)
{
    __shared__ int s_diag[kSeedMaxDiag][64];             // the lane's diagonals, ascending, [entry][lane]
    const int lane = threadIdx.x;
    const int slot = blockIdx.x * 64 + lane;
    const bool real = a.perm[slot] >= 0;
    u32 E0[NWD], E1[NWD], E2[NWD], E3[NWD];
    {
        const size_t pb = (size_t)blockIdx.x * 4 * NWD * 64 + lane;
#pragma unroll
        for (int d = 0; d < NWD; ++d) {
            E0[d] = a.peq[pb + (size_t)(0 * NWD + d) * 64];
            E1[d] = a.peq[pb + (size_t)(1 * NWD + d) * 64];
            E2[d] = a.peq[pb + (size_t)(2 * NWD + d) * 64];
            E3[d] = a.peq[pb + (size_t)(3 * NWD + d) * 64];
        }
    }
    const int m = a.qlen[slot];
    const int T = a.targetLength;
    const int k = a.k;
    // the read as a 2-bit stream (16 symbols per dword) and the rows where it has a symbol of the target
    u32 qs[2 * NWD], V[NWD];
#pragma unroll
    for (int d = 0; d < NWD; ++d) {
        const u32 lo = E1[d] | E3[d], hi = E2[d] | E3[d];
        qs[2 * d] = spread16(lo) | (spread16(hi) << 1);
        qs[2 * d + 1] = spread16(lo >> 16) | (spread16(hi >> 16) << 1);
        V[d] = E0[d] | E1[d] | E2[d] | E3[d];
    }
    bool back = false;
    int nd = 0;                                         // distinct diagonals in s_diag
    const int p = k + 1, L = m / p, r = m % p;
    if (real && L < kSeedQ) back = true;
    for (int i = 0; i < p && real && !back; ++i) {
        const int o = i * L + min(i, r), len = L + (i < r ? 1 : 0);
        // a piece holding a byte the target lacks cannot occur (its rows are empty there)
        bool absent = false;
#pragma unroll
        for (int d = 0; d < NWD; ++d) {
            const int lo = min(max(o - 32 * d, 0), 32), hi = min(max(o + len - 32 * d, 0), 32);
            const u32 mask = hi <= lo ? 0u : (hi - lo >= 32 ? ~0u : (((1u << (hi - lo)) - 1u) << lo));
            if (~V[d] & mask) absent = true;
        }
        if (absent) continue;
        const int w = o >> 4;
        const u32 key = stream_bits(pick(qs, w), pick(qs, w + 1), (u32)o) & ((1u << (2 * kSeedQ)) - 1u);
        const u32 b0 = a.seedOff[key], b1 = a.seedOff[key + 1];
        if (b1 - b0 > (u32)kSeedBucketCap) { back = true; break; }
        for (u32 e = b0; e < b1 && !back; ++e) {
            const int P = (int)a.seedPos[e];
            if (P + len > T) continue;
            bool eq = true;
            for (int j = kSeedQ; j < len && eq; j += 16) {
                const int n = min(16, len - j);
                const u32 mask = n == 16 ? ~0u : ((1u << (2 * n)) - 1u);
                const int x = o + j, y = P + j;
                const u32 qv = stream_bits(pick(qs, x >> 4), pick(qs, (x >> 4) + 1), (u32)x);
                const u32 tv = stream_bits(a.tpk[y >> 4], a.tpk[(y >> 4) + 1], (u32)y);
                eq = ((qv ^ tv) & mask) == 0;
            }
            if (!eq) continue;
            // insert P - o into the ascending list unless it is there
            const int delta = P - o;
            int t = nd;
            while (t > 0 && s_diag[t - 1][lane] > delta) --t;
            if (t > 0 && s_diag[t - 1][lane] == delta) continue;
            if (nd == kSeedMaxDiag) { back = true; break; }
            for (int u = nd; u > t; --u) s_diag[u][lane] = s_diag[u - 1][lane];
            s_diag[t][lane] = delta;
            ++nd;
        }
    }
    // merged windows: a window longer than kSeedMaxWindow hands the read back before anything is scanned
    if (real && !back) {
        int wa = 0, wb = -2;
        for (int t = 0; t < nd && !back; ++t) {
            const int d = s_diag[t][lane];
            const int lo = max(0, d - k), hi = min(T - 1, d + m - 1 + k);
            if (lo <= wb + 1) wb = max(wb, hi);
            else { wa = lo; wb = hi; }
            if (wb - wa + 1 > kSeedMaxWindow) back = true;
        }
    }
    // verification: each merged window from a fresh column (row -1 = 0: HW), the bottom row followed at bit (m - 1) % 32
    int best = k, cnt = 0, cols = 0;
    int* pos = a.pos + (size_t)slot * 16;
    if (real && !back) {
        const u32 sh = (u32)(m - 1) & 31u;
        int t = 0;
        while (t < nd) {
            const int d0 = s_diag[t][lane];
            const int wa = max(0, d0 - k);
            int wb = min(T - 1, d0 + m - 1 + k);
            for (++t; t < nd; ++t) {
                const int d = s_diag[t][lane];
                if (max(0, d - k) > wb + 1) break;
                wb = max(wb, min(T - 1, d + m - 1 + k));
            }
            u32 Pv[NWD], Mv[NWD];
#pragma unroll
            for (int dd = 0; dd < NWD; ++dd) { Pv[dd] = ~0u; Mv[dd] = 0u; }
            int score = m;
            u32 tw = a.tpk[wa >> 4] >> (2 * (wa & 15));
            for (int c = wa; c <= wb; ++c) {
                if ((c & 15) == 0) tw = a.tpk[c >> 4];
                const u32 sym = tw & 3u;
                tw >>= 2;
                u32 Eq[NWD];
#pragma unroll
                for (int dd = 0; dd < NWD; ++dd) Eq[dd] = sym == 0 ? E0[dd] : sym == 1 ? E1[dd] : sym == 2 ? E2[dd] : E3[dd];
                column_step<NWD, 2>(Eq, Pv, Mv, score, sh);
                if (score <= best) {                                   // scan_reads_kernel's EDLIB_AMD_TRACK
                    if (score < best) { best = score; cnt = 0; }
                    if (cnt < 16) pos[cnt] = c;
                    ++cnt;
                }
            }
            cols += wb - wa + 1;
        }
    }
    if (!back) {                                        // a handed-back slot is written by the banded scan's merge
        a.best[slot] = cnt > 0 ? best : -1;
        a.total[slot] = cnt;
        a.flags[slot] = cnt > 16 ? 1 : 0;
    }
    // the hand-back list: one atomic per wave
    const u64 bal = __builtin_amdgcn_ballot_w64(back);
    if (bal) {
        const int first = __builtin_ctzll(bal);
        int base = 0;
        if (lane == first) base = atomicAdd(a.backCount, __popcll(bal));
        base = __builtin_amdgcn_readlane(base, first);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
        if (back) a.backSlots[base + rank] = slot;
    }
    // word-columns verified, summed over the wave
    for (int off = 32; off; off >>= 1) cols += __shfl_xor(cols, off);
    if (lane == 0 && cols > 0) atomicAdd(a.wordSteps, (u64)cols * NWD);
}

hipError_t launch_seed_verify(int nwords, const SeedArgs& a, hipStream_t stream)
{
    if (a.nslots == 0) return hipSuccess;
    const dim3 grid(a.nslots / 64), block(64);
    switch (nwords) {
#define CASE(N) case N: hipLaunchKernelGGL(seed_verify_kernel<N>, grid, block, 0, stream, a); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------ slot lists

namespace {
struct OpenSlot {
    const int *perm, *total, *qlen; int kcfg, kDone, mates;
    __device__ bool operator()(int s) const
    {
        if (perm[s] < 0 || total[s] > 0) return false;
        if (mates && total[s ^ 1] > 0) return false;      // both strands: the mate resolved at a threshold this slot missed
        const int m = qlen[s];
        return (kcfg < 0 ? m : min(m, kcfg)) > kDone;
    }
};
struct FlaggedSlot {
    const int *perm, *flags, *win;                        // win (both strands): strands.hpp's code of the pair s >> 1
    __device__ bool operator()(int s) const
    {
        if (flags[s] == 0 || perm[s] < 0) return false;
        return !win || (win[s >> 1] & 1) == (s & 1);      // a slot whose mate is reported never shows its list
    }
};
}  // namespace

hipError_t select_slots_scratch_bytes(int nslots, size_t* bytes)
{
    size_t a = 0, b = 0;
    hipError_t e = rocprim::select(nullptr, a, rocprim::counting_iterator<int>(0), (int*)nullptr, (int*)nullptr, (size_t)nslots,
                                   OpenSlot{});
    if (e != hipSuccess) return e;
    e = rocprim::select(nullptr, b, rocprim::counting_iterator<int>(0), (int*)nullptr, (int*)nullptr, (size_t)nslots,
                        FlaggedSlot{});
    *bytes = a > b ? a : b;
    return e;
}

hipError_t launch_select_open_slots(const int* perm, const int* total, const int* qlen, int kcfg, int kDone, int nslots,
                                    int* out, int* count, void* tmp, size_t tmpBytes, hipStream_t stream, bool mates)
{
    size_t bytes = tmpBytes;
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<int>(0), out, count, (size_t)nslots,
                           OpenSlot{perm, total, qlen, kcfg, kDone, mates ? 1 : 0}, stream);
}

hipError_t launch_select_flagged_slots(const int* perm, const int* flags, int nslots, int* out, int* count,
                                       void* tmp, size_t tmpBytes, hipStream_t stream, const int* win)
{
    size_t bytes = tmpBytes;
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<int>(0), out, count, (size_t)nslots,
                           FlaggedSlot{perm, flags, win}, stream);
}

__global__ void __launch_bounds__(256)
pick_slot_records_kernel(const int* __restrict__ slots, int n, const int* __restrict__ flags, const int* __restrict__ total,
                         int* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    out[3 * i] = s; out[3 * i + 1] = flags[s]; out[3 * i + 2] = total[s];
}

hipError_t launch_pick_slot_records(const int* slots, int n, const int* flags, const int* total, int* out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pick_slot_records_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, slots, n, flags, total, out);
    return hipGetLastError();
}

}  // namespace edlib_amd
