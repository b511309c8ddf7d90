// reads_seed.hpp -- the seed + verify kernel of the exact k-mer seed filter (reads_seed.hip has the argument and the index) as a
// template, so that its HITS variant (reads_hits.hip) is compiled in a translation unit of its own.
#pragma once
#include "reads_kernels.hpp"
#include "reads_scan.hpp"

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

// ------------------------------------------------------------ seed + verify

// HITS (hit-list read batches): same lookups, caps, de-duplication, window merge and hand-back; the window's
// column loop follows the maximal runs of columns scoring <= k instead of the best-16 record and appends each to a.hits.  A
// window holds every column with D <= k and the column before / behind it scores above k, so no run leaves its window.
template <int NWD, bool HITS = false>
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
            int rFirst = 0, rLast = -2, rMin = 0, rPos = 0, rCnt = 0;   // HITS: the open run (rLast < 0: none)
            auto appendRun = [&] {
                hit_list_append<4>(a.hits, true, [&] { return ((u64)(u32)(a.slotBase + slot) << 32) | (u32)rFirst; },
                                   {rLast, rMin, rPos, rCnt});
            };
            u32 tw = a.tpk[wa >> 4] >> (2 * (wa & 15));
            for (int c = wa; c <= wb; ++c) {
                if ((c & 15) == 0) tw = a.tpk[c >> 4];
                const u32 sym = tw & 3u;
                tw >>= 2;
                u32 Eq[NWD];
#pragma unroll
                for (int dd = 0; dd < NWD; ++dd) Eq[dd] = sym == 0 ? E0[dd] : sym == 1 ? E1[dd] : sym == 2 ? E2[dd] : E3[dd];
                column_step<NWD, 2>(Eq, Pv, Mv, score, sh);
                if constexpr (HITS) {
                    if (score <= k) {
                        const bool fresh = rLast < 0, better = fresh || score < rMin;
                        rFirst = fresh ? c : rFirst;
                        rCnt = better ? 1 : rCnt + (score == rMin ? 1 : 0);
                        rPos = better ? c : rPos;
                        rMin = better ? score : rMin;
                        rLast = c;
                    } else if (rLast >= 0) {
                        appendRun();
                        rLast = -2;
                    }
                } else
                if (score <= best) {                                   // scan_reads_kernel's EDLIB_AMD_TRACK
                    if (score < best) { best = score; cnt = 0; }
                    if (cnt < 16) pos[cnt] = c;
                    ++cnt;
                }
            }
            if constexpr (HITS) if (rLast >= 0) appendRun();
            cols += wb - wa + 1;
        }
    }
    if (!HITS && !back) {                               // a handed-back slot is written by the banded scan's merge
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

}  // namespace edlib_amd
