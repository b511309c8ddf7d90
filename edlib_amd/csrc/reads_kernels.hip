// reads_kernels.hip -- gfx950 kernels for "many short queries, one shared target".
//
// Replaces, for BASELINE.json configs 2/3, the reference's per-query call of
// myersCalcEditDistanceSemiGlobal (edlib.cpp:550-704) + buildPeq (:358-384) +
// calculateBlock (:412-447) and the k-doubling loop around it (:197-217).  Design:
//
//   * one wave64 = 64 queries ("slots") x one segment of the target; every
//     lane owns one query, so the target symbol of a column is WAVE-UNIFORM:
//     it comes from the packed target as a scalar and picks which of the lane's
//     Peq rows feeds the column -- in the banded kernel the target is stored as
//     the LDS row offset itself (16 bits per column, s_load_dwordx8) and goes
//     into M0 with one scalar instruction for a ds_read_addtid_b32 (4, 8 or 16
//     rows per word: targets of up to 16 symbols); in the plain kernel a scalar
//     4-way branch over register rows (2-bit packed target, four symbols).  No
//     cross-lane traffic and no divergence in the DP itself.
//   * the query column lives in VGPRs as NWD 32-bit words (Pv, Mv) instead of
//     the reference's 64-bit blocks: 150 rows need 5 words (160 rows) rather
//     than 3 blocks (192 rows).  The 64-bit add of calculateBlock becomes a
//     v_add_co/v_addc_co carry chain, the <<1 a v_alignbit chain, and every
//     3-input boolean a single v_bitop3_b32 (gfx950).  10 VALU ops per word
//     per column.
//   * the score of the bottom query row is followed directly at bit (m-1) of
//     the last word, so no wildcard padding (the reference's W) is needed and
//     end positions are produced un-shifted.
//     (The dense last level of HW builds its rows bottom-aligned instead: pad rows that
//     match every symbol sit ABOVE the query, where HW keeps them at zero, and the followed
//     row is bit 31 of the last word in every lane -- scan_reads_kernel<NWD, 2, true>.)
//   * HW is shift-invariant: a segment that starts 2m-1 columns early from the
//     fresh state reproduces the exact bottom-row scores of its own columns,
//     so the target is cut into segments for load balance and for small
//     batches; merge_segments() joins them.
//
// Two scan kernels:
//   scan_reads_kernel<NWD, MODE, BOTTOM> every row of every column (SHW, NW; HW for the leftovers of the
//                                       k-doubling whose band is the whole query, and with EDLIB_AMD_BAND=0).
//                                       All outputs are functions of the full DP matrix, so no band is
//                                       needed for correctness and the kernel never branches on data.
//   scan_reads_banded_kernel<NWD, S>    HW: Ukkonen band per wave + k-doubling (the bench kernel, §3b); one wave per
//                                       workgroup, S = 4 / 8 / 16 Peq rows per word.
#include "reads_kernels.hpp"
#include "reads_scan.hpp"
#include "reads_column_asm.hpp"

namespace edlib_amd {

// ------------------------------------------------------------ target packing

__global__ void __launch_bounds__(256)
pack_target_2bit_kernel(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ lut,
                        int T, u32* __restrict__ tpk, int nwords)
{
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const int base = w * 16;
    u32 out = 0;
    if (base + 16 <= T) {
        const uint4 v = *reinterpret_cast<const uint4*>(raw + base);   // 16 B per lane, coalesced
        const u32 d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i)
            out |= (u32)(s_lut[(d[i >> 2] >> ((i & 3) * 8)) & 0xFF] & 3) << (2 * i);
    } else {
        for (int i = 0; i < 16 && base + i < T; ++i)
            out |= (u32)(s_lut[raw[base + i]] & 3) << (2 * i);
    }
    tpk[w] = out;
}

// Expanded target for the banded kernel: 16 bits per column = LDS row offset of the column's Peq rows
// (symbol << 8), so that one scalar instruction per column puts it into M0.  32 columns per thread.
__global__ void __launch_bounds__(256)
pack_target_rows_kernel(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ lut, int T,
                        u32* __restrict__ trows, int ndwords)
{
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int w = blockIdx.x * blockDim.x + threadIdx.x;               // dword = 2 columns
    if (w >= ndwords) return;
    const int c = 2 * w;
    const u32 a0 = c < T ? (u32)(s_lut[raw[c]] & 15) : 0u, a1 = c + 1 < T ? (u32)(s_lut[raw[c + 1]] & 15) : 0u;
    trows[w] = (a0 << 8) | (a1 << 24);
}

hipError_t launch_pack_target_rows(const uint8_t* raw, const uint8_t* lut, int T, u32* trows, int ndwords,
                                   hipStream_t stream)
{
    if (ndwords == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_target_rows_kernel, dim3((ndwords + 255) / 256), dim3(256), 0, stream,
                       raw, lut, T, trows, ndwords);
    return hipGetLastError();
}

hipError_t launch_pack_target_2bit(const uint8_t* raw, const uint8_t* lut, int T, u32* tpk,
                                   hipStream_t stream)
{
    const int nwords = (T + 15) / 16;
    if (nwords == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_target_2bit_kernel, dim3((nwords + 255) / 256), dim3(256), 0, stream,
                       raw, lut, T, tpk, nwords);
    return hipGetLastError();
}

// ------------------------------------------------------------------ buildPeq

// reference buildPeq (edlib.cpp:358-384) restricted to the (<= 16) symbols of the
// target: bit i of row s says "query[i] equals target symbol s".  eqtbl[byte] is
// the 16-bit set of target symbols a query byte equals (identity plus
// additionalEqualities, edlib.cpp:63-94).  Rows at or past the query end stay 0.
// Output layout [readBlock][sym (S = 4, 8 or 16)][word][lane]: a wave loads a row as one 256 B line.
//
// One wave builds the rows of its 64 reads COOPERATIVELY: for read j the lanes load 64 consecutive query bytes
// (one coalesced line), look their symbol sets up, and a ballot per symbol IS the two 32-bit Peq words of those 64
// rows, which lane j keeps.  (Round 1 gave every lane its own read and walked it byte
// by byte: 64 different lines per load instruction, 8.9 GB of fetch per 1M reads against 150 MB of queries.)
// Symbols are done four at a time (4 x NWD row registers); the query bytes are re-read per group from L1 / L2.
// bottomAlign (the rows scan_reads_kernel<NWD, 2, true> reads): query row i goes to bit pad + i, pad = 32 NWD - m, so that
// row m-1 is bit 31 of the last word, and the pad bits below are set in the row of every symbol.  pad is below 32 for the
// reads of a group (read_group_words: they reach into the last word); the padding slots of a list (m = 1) and any shorter
// read get whole words of pad the same way, nothing here or in the scan's initial state assumes pad < 32.
// bottomAlign = 1 + R (R = 3 or 7; scan_reads_kernel<NWD, 2, true, R>): R delay rows above row m-1, set in the row of every
// symbol like the pads, and pad = 32 NWD - R - m: row m-1 is bit 31 - R of the last word.  The caller sees to m + R <= 32 NWD.
template <int NWD>
__global__ void __launch_bounds__(256)
build_peq_reads_kernel(const uint8_t* __restrict__ reads, const long long* __restrict__ qoff,
                       const int* __restrict__ perm, int nslots, int S,
                       const uint16_t* __restrict__ eqtbl, const u32* __restrict__ tpres, int kcfg,
                       u32* __restrict__ peq, int* __restrict__ qlen, int* __restrict__ kinit,
                       int* __restrict__ alphaExtra, int bottomAlign)
{
    __shared__ uint16_t s_eq[256];
    s_eq[threadIdx.x] = eqtbl[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);               // read block of this wave
    if (blk * 64 >= nslots) return;
    const int slot = blk * 64 + lane;
    const int r = slot < nslots ? perm[slot] : -1;
    long long off = 0; int m = 1;
    if (r >= 0) { off = qoff[r]; m = (int)(qoff[r + 1] - off); }
    int extra = 0;
    for (int g0 = 0; g0 < S; g0 += 4) {
        u32 E[4][NWD];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int d = 0; d < NWD; ++d) E[s][d] = 0;
        for (int j = 0; j < 64; ++j) {                                 // read j of the wave (wave-uniform)
            const int rj = __builtin_amdgcn_readlane(r, j);
            if (rj < 0) continue;
            const int mj = __builtin_amdgcn_readlane(m, j);
            const long long offj = ((long long)__builtin_amdgcn_readlane((int)(off >> 32), j) << 32)
                                 | (u32)__builtin_amdgcn_readlane((int)off, j);
            // bytes of this read that do not occur in the target, counted once each (alphabetLength): wave-uniform
            // 256-bit set, only touched when a lane holds such a byte (first symbol group only)
            unsigned long long seen0 = 0, seen1 = 0, seen2 = 0, seen3 = 0;
            int extraJ = 0;
            const bool mine = lane == j;                               // the lane that keeps read j's rows
            const int delay = bottomAlign > 1 ? bottomAlign - 1 : 0;
            const int padj = bottomAlign ? 32 * NWD - delay - mj : 0;  // wave-uniform
#pragma unroll
            for (int c = 0; c < (NWD + 1) / 2; ++c) {                  // 64 rows = two words per trip
                const int i = 64 * c + lane - padj;                    // query row of bit 64 c + lane
                const bool in = i >= 0 && i < mj;
                const u32 by = in ? reads[offj + i] : 0u;
                const u32 mask = in ? ((u32)s_eq[by] >> g0) : ((i < 0 || i < mj + delay) ? 0xfu : 0u);   // pad and delay rows match every symbol
                const unsigned long long b0 = __builtin_amdgcn_ballot_w64((mask & 1u) != 0), b1 = __builtin_amdgcn_ballot_w64((mask & 2u) != 0);
                const unsigned long long b2 = __builtin_amdgcn_ballot_w64((mask & 4u) != 0), b3 = __builtin_amdgcn_ballot_w64((mask & 8u) != 0);
                constexpr int w0 = 0;
                const int d0 = 2 * c, d1 = (2 * c + 1 < NWD) ? 2 * c + 1 : w0;
                E[0][d0] = (mine ? (u32)b0 : E[0][d0]); E[1][d0] = (mine ? (u32)b1 : E[1][d0]);
                E[2][d0] = (mine ? (u32)b2 : E[2][d0]); E[3][d0] = (mine ? (u32)b3 : E[3][d0]);
                if (2 * c + 1 < NWD) {
                    E[0][d1] = (mine ? (u32)(b0 >> 32) : E[0][d1]); E[1][d1] = (mine ? (u32)(b1 >> 32) : E[1][d1]);
                    E[2][d1] = (mine ? (u32)(b2 >> 32) : E[2][d1]); E[3][d1] = (mine ? (u32)(b3 >> 32) : E[3][d1]);
                }
                if (g0 == 0) {
                    unsigned long long np = __builtin_amdgcn_ballot_w64(in && !((tpres[by >> 5] >> (by & 31)) & 1u));
                    while (np) {                                       // rare: a query byte the target does not have
                        const int l = __builtin_ctzll(np);
                        const u32 v = (u32)__builtin_amdgcn_readlane((int)by, l);
                        const unsigned long long bit = 1ull << (v & 63);
                        unsigned long long& sw = (v >> 6) == 0 ? seen0 : (v >> 6) == 1 ? seen1 : (v >> 6) == 2 ? seen2 : seen3;
                        if (!(sw & bit)) { sw |= bit; ++extraJ; }
                        np &= ~__builtin_amdgcn_ballot_w64(in && by == v);
                    }
                }
            }
            if (g0 == 0 && mine) extra = extraJ;
        }
        if (slot < nslots) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int d = 0; d < NWD; ++d)
                    peq[((size_t)(blk * S + g0 + s) * NWD + d) * 64 + lane] = E[s][d];
        }
    }
    if (slot >= nslots) return;
    qlen[slot] = m;
    // candidates are columns scoring <= min(k, m): HW clamps k to m (edlib.cpp:566-568) and
    // for SHW the best score never exceeds m either (the empty prefix costs m)
    kinit[slot] = (kcfg < 0 || kcfg > m) ? m : kcfg;
    alphaExtra[slot] = extra;
}

template <int NWD>
static hipError_t launch_build_peq_t(const uint8_t* reads, const long long* qoff, const int* perm,
                                     int nslots, int S, const uint16_t* eqtbl, const u32* tpres, int kcfg,
                                     u32* peq, int* qlen, int* kinit, int* alphaExtra,
                                     hipStream_t stream, int bottomAlign)
{
    hipLaunchKernelGGL(build_peq_reads_kernel<NWD>, dim3((nslots + 255) / 256), dim3(256), 0, stream,
                       reads, qoff, perm, nslots, S, eqtbl, tpres, kcfg, peq, qlen, kinit, alphaExtra, bottomAlign);
    return hipGetLastError();
}

hipError_t launch_build_peq_reads(int nwords, int syms, const uint8_t* reads, const long long* qoff,
                                  const int* perm, int nslots, const uint16_t* eqtbl,
                                  const u32* tpres, int kcfg, u32* peq, int* qlen, int* kinit,
                                  int* alphaExtra, hipStream_t stream, int bottomAlign)
{
    if (nslots == 0) return hipSuccess;
    if (!bottom_align_valid(bottomAlign)) return hipErrorInvalidValue;
    if (syms != 4 && syms != 8 && syms != 16) return hipErrorInvalidValue;
    switch (nwords) {
#define CASE(N) case N: return launch_build_peq_t<N>(reads, qoff, perm, nslots, syms, eqtbl, tpres, kcfg, peq, qlen, kinit, alphaExtra, stream, bottomAlign);
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(10) CASE(12) CASE(14) CASE(16) CASE(24) CASE(32)
#undef CASE
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------- the scan

// The distinct asm comments keep the four bodies from being tail-merged back
// into one body fed by v_mov/v_cndmask of the Peq row.
#define EDLIB_AMD_DISPATCH_COLUMN(sym)                                                     \
    switch (sym) {                                                                         \
        case 0:  column_step<NWD, MODE, BOTTOM>(E0, Pv, Mv, score, sh, zr0, zr1); asm volatile("; sym0"); break; \
        case 1:  column_step<NWD, MODE, BOTTOM>(E1, Pv, Mv, score, sh, zr0, zr1); asm volatile("; sym1"); break; \
        case 2:  column_step<NWD, MODE, BOTTOM>(E2, Pv, Mv, score, sh, zr0, zr1); asm volatile("; sym2"); break; \
        default: column_step<NWD, MODE, BOTTOM>(E3, Pv, Mv, score, sh, zr0, zr1); asm volatile("; sym3"); break; \
    }

#define EDLIB_AMD_DISPATCH_COLUMN_DELAY(FORM, sym)                                         \
    switch (sym) {                                                                         \
        case 0:  column_step_delay<NWD, FORM, R>(E0, Pv, Mv, score, nph, nmh, zr0, zr1); asm volatile("; sym0"); break; \
        case 1:  column_step_delay<NWD, FORM, R>(E1, Pv, Mv, score, nph, nmh, zr0, zr1); asm volatile("; sym1"); break; \
        case 2:  column_step_delay<NWD, FORM, R>(E2, Pv, Mv, score, nph, nmh, zr0, zr1); asm volatile("; sym2"); break; \
        default: column_step_delay<NWD, FORM, R>(E3, Pv, Mv, score, nph, nmh, zr0, zr1); asm volatile("; sym3"); break; \
    }

// Record column `col` if it ties or improves the best bottom-row score
// (reference edlib.cpp:658-673: "colScore <= k", "positions.clear()", "k = bestScore").
#define EDLIB_AMD_TRACK_SCORE(sc, col)                         \
    if ((sc) <= best) {                                        \
        if ((sc) < best) { best = (sc); cnt = 0; }             \
        if (cnt < cap) pos[cnt] = (col);                       \
        ++cnt;                                                 \
    }
#define EDLIB_AMD_TRACK(col) EDLIB_AMD_TRACK_SCORE(score, col)

// BOTTOM (HW): the Peq rows were built bottom-aligned (build_peq_reads_kernel), query row r at bit 32 NWD - m + r.  The
// pad rows below bit 32 NWD - m match every symbol; with HW's zero row -1 they stay at D = 0 in every column, so the real
// rows see the boundary they always saw, and the followed row m-1 is bit 31 of the last word in every lane.
// R > 0 (with BOTTOM): the rows carry R = 3 or 7 all-match rows above row m-1 (bit 31 - R of the last word).  Each copies the
// row above it one column late, so the top R + 1 bits of the LAST column of a group of R + 1 are the followed row's deltas of
// the whole group: R columns of a group carry no score code, the last hands out the two nibbles (bytes at R = 7), and the score
// moves once per group, by two popcounts (tests/delay_rows_model.py and tests/delay_rows8_model.py have the identity and its
// boundaries).
template <int NWD, int MODE, bool BOTTOM = false, int R = 0>
__global__ void __launch_bounds__(256)
scan_reads_kernel(const ReadScanArgs a)
{
    constexpr bool DELAY = R > 0;
    static_assert(R == 0 || R == kDelayRowsShallow || R == kDelayRowsDeep, "delay rows: none, three or seven");
    static_assert(!DELAY || (BOTTOM && MODE == 2), "delay rows: bottom-aligned HW rows");
    constexpr int kHitGroup = DELAY ? R + 1 : 4;                   // columns per hit test (divides 16): one nibble or byte per group
    static_assert(16 % kHitGroup == 0, "no group straddles a 16-column target word");
    const int lane = threadIdx.x & 63;
    const int rblk = blockIdx.x * 4 + (threadIdx.x >> 6);          // 4 waves / workgroup
    const int seg = blockIdx.y;
    const int idx = rblk * 64 + lane;                              // lane index in this launch
    if (rblk * 64 >= a.nlanes) return;                             // whole wave out of range
    const bool live = idx < a.nlanes;
    const int slot = live ? (a.slotmap ? a.slotmap[idx] : idx) : 0;
#ifdef EDLIB_AMD_DRAIN_DIAG
    // diagnostic build only (tools/drain_model.py): when every wave of the launch came and went.  (The wave's index is worked
    // out again at the exit from what the loop keeps anyway: a register held across the scan would cost the kernel a wave.)
    if (BOTTOM && a.waveClock && lane == 0)
        a.waveClock[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)] = wall_clock64();
#endif

    u32 E0[NWD], E1[NWD], E2[NWD], E3[NWD], Pv[NWD], Mv[NWD];
    {
        const size_t pb = (size_t)(slot >> 6) * 4 * NWD * 64 + (slot & 63);
#pragma unroll
        for (int d = 0; d < NWD; ++d) {
            E0[d] = a.peq[pb + (size_t)(0 * NWD + d) * 64];
            E1[d] = a.peq[pb + (size_t)(1 * NWD + d) * 64];
            E2[d] = a.peq[pb + (size_t)(2 * NWD + d) * 64];
            E3[d] = a.peq[pb + (size_t)(3 * NWD + d) * 64];
            Pv[d] = ~0u;                                           // column -1: D[i][-1] = i+1 (edlib.cpp:575-579)
            Mv[d] = 0u;
        }
    }
    const int m = a.qlen[slot];
    if constexpr (BOTTOM) {
        // column -1 of the pad rows is 0: Pv is clear on the 32 NWD - m low bits.  Reads of a group fill their last word
        // (read_group_words), so the pad is below 32 there; the padding slots of the rebuilt rows (m = 1) and anything
        // shorter still get whole words of pad.
        const int pad = 32 * NWD - R - m;                          // (delay rows: Pv = 1, D[i][-1] = i + 1 like the read's own)
#pragma unroll
        for (int d = 0; d < NWD; ++d) {
            const int lo = pad - 32 * d;
            Pv[d] = lo <= 0 ? ~0u : (lo >= 32 ? 0u : ~0u << lo);
        }
    }
    const u32 sh = (u32)(m - 1) & 31u;
    // the pair form of the bottom-aligned column (reads_column_asm.hpp) adds its carries as (carry, 0) register pairs: the
    // zeros of the two high halves stand in registers through the whole scan (opaque and apart, so that neither is
    // rematerialised or copied per column)
    u32 zr0 = 0, zr1 = 0;
    if constexpr (BOTTOM && (NWD == 4 || NWD == 5)) {
        asm volatile("v_mov_b32 %0, 0" : "=v"(zr0));
        asm volatile("v_mov_b32 %0, 0" : "=v"(zr1));
    }
    int score = m;
    int best = a.kinit[slot];
    int cnt = 0;
    const long long item = (long long)idx * a.numSegments + seg;   // (lane, segment) record
    // lanes past nlanes (the tail of the last wave) own no record: they must not even read the tables
    const int cap = !live ? 0 : (a.posCap ? a.posCap[item] : a.cap);
    int* pos = a.segPos + (!live ? 0 : (a.posOff ? a.posOff[item] : item * a.cap));
    // The lane's running best over all its segments (ReadScanArgs::liveBest).  Results do not depend on when a segment sees
    // what another one found: liveBest only ever holds the lane's threshold or a score that some column reaches, so it is
    // never below the read's minimum over the whole target, and under ANY bound at or above that minimum a segment records
    // every one of its columns that scores the minimum, in order, counting past the cap (a lower score first clears what
    // was recorded above it, an import does the same, and nothing at the minimum is ever cleared: no import is below it).
    // A segment without such a column ends above the minimum, or at it with a count of 0; the merge takes neither.
    constexpr int kLiveBlocks = kLivePeriod / 16;
    constexpr int kNoImport = 0x1fffffff;                          // (twice this and a few more is still an int)
    int* const livep = BOTTOM ? a.liveBest : nullptr;              // wave-uniform
    // (the loop keeps ONE register for the lane's index, opaque so that the 64-bit record index is not kept beside it: the
    // final stores work theirs out again)
    int lidx = idx;
    if constexpr (BOTTOM) asm volatile("" : "+v"(lidx));
#define EDLIB_AMD_LIVE_LOAD() (live ? __hip_atomic_load(livep + lidx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kNoImport)

    const int T = a.targetLength;
    int c0 = seg * a.segLen, c1 = c0 + a.segLen;                   // c0: multiple of 16
    if (a.segTable) { const Segment sg = a.segTable[seg]; c0 = sg.start; c1 = c0 + sg.cols; }   // (one scalar load per wave)
    if (c1 > T) c1 = T;
    int cw = c0 - a.warm; if (cw < 0) cw = 0;
    cw &= ~15;

    // warm-up columns [cw, c0): state only, nothing is recorded (HW segments)
    u32 nph = 0, nmh = 0;                                          // DELAY: the nibbles / bytes of the last group
    for (int w = cw >> 4; w < (c0 >> 4); ++w) {
        const u32 tw = a.tpk[w];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const u32 sym = (tw >> (2 * j)) & 3u;
            if constexpr (!DELAY) {
                EDLIB_AMD_DISPATCH_COLUMN(sym)
            } else if ((j & (kHitGroup - 1)) != kHitGroup - 1) {
                EDLIB_AMD_DISPATCH_COLUMN_DELAY(0, sym)
            } else {
                EDLIB_AMD_DISPATCH_COLUMN_DELAY(1, sym)
            }
        }
    }
    // full words of the segment
    const int wend = c1 >> 4;
    // The hit test runs once per group of kHitGroup columns: bottom-row scores of neighbouring columns differ by at most 1,
    // so a last score above best + kHitGroup - 1 means that no column of the group is at or below best, and best only moves
    // at a hit.  A group that may hold one goes through the per-column test, in order, with each column's own score: best,
    // cnt and the stored positions are what the per-column test leaves.  (Unrelated reads sit ~14 above their best: a lane
    // passes in about 0.5 % of its groups, a wave of 64 in three of ten.)  The loop carries the limit, not best: one compare per group.
    int lim = best + (kHitGroup - 1);
    if constexpr (DELAY) {
        // The capture column leaves the score of the group's last column next to the one before the group.  With b and a
        // the scores before and after a group of G = kHitGroup columns, its column k = 1..G scores at least
        // max(b - k, a - (G - k)) >= (a + b - G) / 2, so a group may hold a hit only when a + b <= 2 best + G: one add and
        // one compare per group, and tighter than a <= best + G - 1 for the reads that hover above their best.  It matters: a
        // WAVE takes the slow path when any of its 64 lanes passes (at four columns, three groups in ten at a <= best + 3).
        // There the G scores come out of the nibbles (bytes), bit 31 the first column of the group, and the per-column test
        // runs only if their least is a hit.
        int lim2 = 2 * best + kHitGroup;
        for (int w0 = c0 >> 4; w0 < wend; w0 += kLiveBlocks) {
        if (livep) {
            // a lower import replaces best, and what was recorded belonged to a score that is no longer the best; an equal
            // one changes nothing, so the ties already recorded stay
            const int got = EDLIB_AMD_LIVE_LOAD();
            if (2 * got + kHitGroup < lim2) { lim2 = 2 * got + kHitGroup; cnt = 0; }
        }
        const int w1 = w0 + kLiveBlocks < wend ? w0 + kLiveBlocks : wend;
        for (int w = w0; w < w1; ++w) {
            const u32 tw = a.tpk[w];
#pragma unroll
            for (int j = 0; j < 16; j += kHitGroup) {
#pragma unroll
                for (int q = 0; q < kHitGroup - 1; ++q) {
                    const u32 sym = (tw >> (2 * (j + q))) & 3u;
                    EDLIB_AMD_DISPATCH_COLUMN_DELAY(0, sym)
                }
                const int before = score;
                {
                    const u32 sym = (tw >> (2 * (j + kHitGroup - 1))) & 3u;
                    EDLIB_AMD_DISPATCH_COLUMN_DELAY(1, sym)
                }
                if (__builtin_expect(score + before <= lim2, 0)) {
                    int sc[kHitGroup], acc = before, least = 0x7fffffff;
#pragma unroll
                    for (int q = 0; q < kHitGroup; ++q) {
                        acc += (int)((nph >> (kHitGroup - 1 - q)) & 1u) - (int)((nmh >> (kHitGroup - 1 - q)) & 1u);
                        sc[q] = acc;
                        least = acc < least ? acc : least;
                    }
                    best = (lim2 - kHitGroup) >> 1;
                    if (least <= best) {
#pragma unroll
                        for (int q = 0; q < kHitGroup; ++q) { EDLIB_AMD_TRACK_SCORE(sc[q], w * 16 + j + q) }
                        if (livep && live && 2 * best + kHitGroup < lim2) atomicMin(livep + lidx, best);   // improved: publish
                        lim2 = 2 * best + kHitGroup;
                    }
                }
            }
        }
        }
        lim = ((lim2 - kHitGroup) >> 1) + (kHitGroup - 1);
    }
    for (int w0 = c0 >> 4; !DELAY && w0 < wend; w0 += kLiveBlocks) {
    if (livep) {
        const int got = EDLIB_AMD_LIVE_LOAD();
        if (got + (kHitGroup - 1) < lim) { lim = got + (kHitGroup - 1); cnt = 0; }
    }
    const int w1 = w0 + kLiveBlocks < wend ? w0 + kLiveBlocks : wend;
    for (int w = w0; w < w1; ++w) {
        const u32 tw = a.tpk[w];
#pragma unroll
        for (int j = 0; j < 16; j += kHitGroup) {
            int sc[kHitGroup];
#pragma unroll
            for (int q = 0; q < kHitGroup; ++q) {
                const u32 sym = (tw >> (2 * (j + q))) & 3u;
                EDLIB_AMD_DISPATCH_COLUMN(sym)
                sc[q] = score;
            }
            if (MODE != 0) {
                if (__builtin_expect(score <= lim, 0)) {
                    best = lim - (kHitGroup - 1);
#pragma unroll
                    for (int q = 0; q < kHitGroup; ++q) { EDLIB_AMD_TRACK_SCORE(sc[q], w * 16 + j + q) }
                    if (livep && live && best + (kHitGroup - 1) < lim) atomicMin(livep + lidx, best);   // improved: publish
                    lim = best + (kHitGroup - 1);
                }
            }
        }
    }
    }
#undef EDLIB_AMD_LIVE_LOAD
    best = lim - (kHitGroup - 1);
    // ragged tail of the target (last segment only)
    const int rem = c1 - (wend << 4);
    if (rem > 0) {
        u32 tw = a.tpk[wend];
        for (int j = 0; j < rem; ++j) {
            const u32 sym = tw & 3u;
            tw >>= 2;
            if constexpr (DELAY) { EDLIB_AMD_DISPATCH_COLUMN_DELAY(2, sym) } else { EDLIB_AMD_DISPATCH_COLUMN(sym) }
            if (MODE != 0) { EDLIB_AMD_TRACK(wend * 16 + j) }
        }
    }
    if (live) {
        const size_t o = (size_t)lidx * a.numSegments + seg;
        a.segBest[o] = (MODE == 0) ? score : best;                 // NW: D[m][T] (edlib.cpp:914-917)
        a.segCnt[o] = (MODE == 0) ? 1 : cnt;
    }
#ifdef EDLIB_AMD_DRAIN_DIAG
    if (BOTTOM && a.waveClock && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {
        const int rb = lidx >> 6;                                  // = rblk
        a.waveClock[((size_t)gridDim.y + blockIdx.y) * gridDim.x * 4 + rb] = wall_clock64();
    }
#endif
}

template <int NWD>
static hipError_t launch_scan_mode(int mode, const ReadScanArgs& a, hipStream_t stream)
{
    const int nrblk = (a.nlanes + 63) / 64;
    dim3 grid((nrblk + 3) / 4, a.numSegments), block(256);
    switch (mode) {
        case 0: hipLaunchKernelGGL((scan_reads_kernel<NWD, 0>), grid, block, 0, stream, a); break;
        case 1: hipLaunchKernelGGL((scan_reads_kernel<NWD, 1>), grid, block, 0, stream, a); break;
        case 2: if (a.bottomAligned == 1 + kDelayRowsDeep) hipLaunchKernelGGL((scan_reads_kernel<NWD, 2, true, kDelayRowsDeep>), grid, block, 0, stream, a);
                else if (a.bottomAligned == 1 + kDelayRowsShallow) hipLaunchKernelGGL((scan_reads_kernel<NWD, 2, true, kDelayRowsShallow>), grid, block, 0, stream, a);
                else if (a.bottomAligned) hipLaunchKernelGGL((scan_reads_kernel<NWD, 2, true>), grid, block, 0, stream, a);
                else hipLaunchKernelGGL((scan_reads_kernel<NWD, 2>), grid, block, 0, stream, a);
                break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scan_reads(int nwords, int mode, const ReadScanArgs& a, hipStream_t stream)
{
    if (a.nlanes == 0) return hipSuccess;
    if (a.bottomAligned && mode != 2) return hipErrorInvalidValue;      // only HW keeps the pad rows at zero
    if (!bottom_align_valid(a.bottomAligned)) return hipErrorInvalidValue;
    switch (nwords) {
#define CASE(N) case N: return launch_scan_mode<N>(mode, a, stream);
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    }
    return hipErrorInvalidValue;
}

template <int NWD>
static hipError_t resident_bottom(int bottomAligned, int* perCU)
{
    if (bottomAligned == 1 + kDelayRowsDeep) return hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, scan_reads_kernel<NWD, 2, true, kDelayRowsDeep>, 256, 0);
    if (bottomAligned == 1 + kDelayRowsShallow) return hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, scan_reads_kernel<NWD, 2, true, kDelayRowsShallow>, 256, 0);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, scan_reads_kernel<NWD, 2, true>, 256, 0);
}

hipError_t scan_reads_resident_workgroups(int nwords, int bottomAligned, int* resident)
{
    int dev = 0, cus = 0, perCU = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    switch (nwords) {
#define CASE(N) case N: e = resident_bottom<N>(bottomAligned, &perCU); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    *resident = perCU * cus;
    return e;
}

// ------------------------------------------------------------- launchers (groups of up to 8 words; longer: reads_kernels_long.hip)

hipError_t launch_scan_reads_full_long(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream);
hipError_t launch_scan_reads_banded_long(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream);

template <int S, bool CHAIN>
static hipError_t launch_scan_reads_full_s(int nwords, const ReadScanArgs& a, hipStream_t stream)
{
    dim3 grid((a.nlanes + 63) / 64, a.numSegments), block(64);
    switch (nwords) {
#define CASE(N) case N: EDLIB_AMD_CHECK_STATIC_LDS((scan_reads_full_kernel<N, S, CHAIN>), N * S * 256); \
                        hipLaunchKernelGGL((scan_reads_full_kernel<N, S, CHAIN>), grid, block, 0, stream, a); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scan_reads_full(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream)
{
    if (a.nlanes == 0) return hipSuccess;
    if (a.segTable) return hipErrorInvalidValue;                        // only scan_reads_kernel reads a table
    if (nwords > kMaxReadWords) return launch_scan_reads_full_long(nwords, syms, a, stream);
    const bool chain = a.chainIn != nullptr || a.chainOut != nullptr;
    switch (syms) {
        case 4: return chain ? launch_scan_reads_full_s<4, true>(nwords, a, stream) : launch_scan_reads_full_s<4, false>(nwords, a, stream);
        case 8: return chain ? launch_scan_reads_full_s<8, true>(nwords, a, stream) : launch_scan_reads_full_s<8, false>(nwords, a, stream);
        case 16: return chain ? launch_scan_reads_full_s<16, true>(nwords, a, stream) : launch_scan_reads_full_s<16, false>(nwords, a, stream);
    }
    return hipErrorInvalidValue;
}

template <int S>
static hipError_t launch_scan_reads_banded_s(int nwords, const ReadScanArgs& a, hipStream_t stream)
{
    const int nrblk = (a.nlanes + 63) / 64;
    dim3 grid(nrblk, a.numSegments), block(64);
    switch (nwords) {
#define CASE(N) case N: if (a.filter) { EDLIB_AMD_CHECK_STATIC_LDS((scan_reads_banded_kernel<N, S, true>), N * S * 256); \
                                            hipLaunchKernelGGL((scan_reads_banded_kernel<N, S, true>), grid, block, 0, stream, a); } \
                        else { EDLIB_AMD_CHECK_STATIC_LDS((scan_reads_banded_kernel<N, S, false>), N * S * 256); \
                               hipLaunchKernelGGL((scan_reads_banded_kernel<N, S, false>), grid, block, 0, stream, a); } break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scan_reads_banded(int nwords, int syms, const ReadScanArgs& a, hipStream_t stream)
{
    if (a.nlanes == 0) return hipSuccess;
    if (a.segTable) return hipErrorInvalidValue;
    if (nwords > kMaxReadWords) return a.filter ? hipErrorInvalidValue : launch_scan_reads_banded_long(nwords, syms, a, stream);
    switch (syms) {
        case 4: return launch_scan_reads_banded_s<4>(nwords, a, stream);
        case 8: return launch_scan_reads_banded_s<8>(nwords, a, stream);
        case 16: return launch_scan_reads_banded_s<16>(nwords, a, stream);
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------- filter candidates

__global__ void __launch_bounds__(256)
collect_candidates_kernel(const int* __restrict__ segCnt, const int* __restrict__ segPos, int S, int cap, int nlanes,
                          int* __restrict__ out, int maxOut, int* __restrict__ counter, int* __restrict__ overflow)
{
    const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;    // (lane, segment) record
    if (item >= (long long)nlanes * S) return;
    const int c = segCnt[item];
    if (c <= 0) return;
    const int lane = (int)(item / S);
    if (c > cap) overflow[lane] = 1;
    const int take = c < cap ? c : cap;
    const int at = atomicAdd(counter, take);
    for (int i = 0; i < take; ++i)
        if (at + i < maxOut) { out[2 * (at + i)] = lane; out[2 * (at + i) + 1] = segPos[item * cap + i]; }
}

hipError_t launch_collect_candidates(const int* segCnt, const int* segPos, int numSegments, int cap, int nlanes,
                                     int* out, int maxOut, int* counter, int* overflow, hipStream_t stream)
{
    const long long items = (long long)nlanes * numSegments;
    if (items == 0) return hipSuccess;
    hipLaunchKernelGGL(collect_candidates_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream,
                       segCnt, segPos, numSegments, cap, nlanes, out, maxOut, counter, overflow);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the merge

// Joins the per-segment records of a slot: global best, number of columns
// attaining it, and the first capFinal positions in ascending order
// (reference semantics of positions_, edlib.cpp:662-671).  flags != 0: the
// list is incomplete and the host runs the exact second pass for that slot.
// 1: a contributing segment holds more hits than its cap (the slot is scanned
// again); gatherFlag: every contributing segment fits and only the final list
// overflowed -- the complete ascending list is in these records, and
// gather_segments_kernel copies it out without a scan (gatherFlag = 1: the
// records will not live that long).  total[] is exact either way: segCnt
// counts the hits past the cap too.
__global__ void __launch_bounds__(256)
merge_segments_kernel(const int* __restrict__ segBest, const int* __restrict__ segCnt,
                      const int* __restrict__ segPos, int S, int cap, int nlanes,
                      const int* __restrict__ slotmap, int capFinal,
                      int* __restrict__ best, int* __restrict__ total, int* __restrict__ pos,
                      int* __restrict__ flags, int gatherFlag)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // lane index of the scan launch
    if (idx >= nlanes) return;
    const int slot = slotmap ? slotmap[idx] : idx;
    const size_t base = (size_t)idx * S;
    int b = 0x7fffffff;
    for (int s = 0; s < S; ++s)
        if (segCnt[base + s] > 0 && segBest[base + s] < b) b = segBest[base + s];
    int n = 0, ovf = 0;
    if (b != 0x7fffffff) {
        for (int s = 0; s < S; ++s) {
            const int c = segCnt[base + s];
            if (c <= 0 || segBest[base + s] != b) continue;
            if (c > cap) ovf = 1;
            const int take = c < cap ? c : cap;
            for (int i = 0; i < take; ++i)
                if (n + i < capFinal) pos[(size_t)slot * capFinal + n + i] = segPos[(base + s) * cap + i];
            n += c;
        }
        if (!ovf && n > capFinal) ovf = gatherFlag;
    }
    best[slot] = (b == 0x7fffffff) ? -1 : b;
    total[slot] = n;
    flags[slot] = ovf;
}

// The same merge with a wave per lane of the scan launch, its lanes striding over the segments: small batches cut the target
// into hundreds of segments (851 leftovers of a 16,384-read batch x 1,216 segments: 0.80 ms with a thread per slot walking
// its 1,216 entries one dependent load after the other).
__global__ void __launch_bounds__(64)
merge_segments_wave_kernel(const int* __restrict__ segBest, const int* __restrict__ segCnt,
                           const int* __restrict__ segPos, int S, int cap, int nlanes,
                           const int* __restrict__ slotmap, int capFinal,
                           int* __restrict__ best, int* __restrict__ total, int* __restrict__ pos,
                           int* __restrict__ flags, int gatherFlag)
{
    const int idx = blockIdx.x, lane = threadIdx.x;
    const int slot = slotmap ? slotmap[idx] : idx;
    const size_t base = (size_t)idx * S;
    int b = 0x7fffffff;
    for (int s = lane; s < S; s += 64)
        if (segCnt[base + s] > 0 && segBest[base + s] < b) b = segBest[base + s];
    for (int off = 32; off; off >>= 1) { const int o = __shfl_xor(b, off); b = o < b ? o : b; }
    int n = 0, ovf = 0;
    if (b != 0x7fffffff) {
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            int c = s < S ? segCnt[base + s] : 0;
            if (c <= 0 || segBest[base + s] != b) c = 0;
            if (c > cap) ovf = 1;
            int incl = c;                                   // inclusive prefix sum over the wave: where this segment's hits go
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            const int at = n + incl - c, take = c < cap ? c : cap;
            for (int i = 0; i < take; ++i)
                if (at + i < capFinal) pos[(size_t)slot * capFinal + at + i] = segPos[(base + s) * cap + i];
            n += __shfl(incl, 63);
        }
        ovf = __any(ovf) ? 1 : 0;
        if (!ovf && n > capFinal) ovf = gatherFlag;
    }
    if (lane == 0) {
        best[slot] = (b == 0x7fffffff) ? -1 : b;
        total[slot] = n;
        flags[slot] = ovf;
    }
}

hipError_t launch_merge_segments(const int* segBest, const int* segCnt, const int* segPos, int S,
                                 int cap, int nlanes, const int* slotmap, int capFinal, int* best,
                                 int* total, int* pos, int* flags, hipStream_t stream, int gatherFlag)
{
    if (nlanes == 0) return hipSuccess;
    if (S >= 64) {
        hipLaunchKernelGGL(merge_segments_wave_kernel, dim3(nlanes), dim3(64), 0, stream,
                           segBest, segCnt, segPos, S, cap, nlanes, slotmap, capFinal, best, total, pos, flags, gatherFlag);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(merge_segments_kernel, dim3((nlanes + 255) / 256), dim3(256), 0, stream,
                       segBest, segCnt, segPos, S, cap, nlanes, slotmap, capFinal, best, total, pos, flags, gatherFlag);
    return hipGetLastError();
}

// The exact pass of a slot whose segments all fit their cap: merge_segments_wave_kernel's prefix sums with the slot's own
// total as the capacity.  A wave per entry; idx = lane of the scan launch that left the records, off / lim = where the list
// goes in `out` and how long it is (the merge's total[]).
__global__ void __launch_bounds__(64)
gather_segments_kernel(const int* __restrict__ segBest, const int* __restrict__ segCnt,
                       const int* __restrict__ segPos, int S, int cap, const int* __restrict__ idx,
                       const long long* __restrict__ off, const int* __restrict__ lim, int* __restrict__ out)
{
    const int lane = threadIdx.x;
    const size_t base = (size_t)idx[blockIdx.x] * S;
    int* dst = out + off[blockIdx.x];
    const int capOut = lim[blockIdx.x];
    int b = 0x7fffffff;
    for (int s = lane; s < S; s += 64)
        if (segCnt[base + s] > 0 && segBest[base + s] < b) b = segBest[base + s];
    for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(b, o); b = t < b ? t : b; }
    if (b == 0x7fffffff) return;
    int n = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        int c = s < S ? segCnt[base + s] : 0;
        if (c <= 0 || segBest[base + s] != b) c = 0;
        int incl = c;
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        const int at = n + incl - c, take = c < cap ? c : cap;
        for (int i = 0; i < take; ++i)
            if (at + i < capOut) dst[at + i] = segPos[(base + s) * cap + i];
        n += __shfl(incl, 63);
    }
}

hipError_t launch_gather_segments(const int* segBest, const int* segCnt, const int* segPos, int S, int cap, int n,
                                  const int* idx, const long long* off, const int* lim, int* out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_segments_kernel, dim3(n), dim3(64), 0, stream, segBest, segCnt, segPos, S, cap, idx, off, lim, out);
    return hipGetLastError();
}

}  // namespace edlib_amd
