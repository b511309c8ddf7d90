// cross_column.hpp -- the column of the lane-per-cell kernels (cross_kernels.hip, window_kernels.hip): a lane owns one
// cell and carries the whole height of its query, at most 8 words of 32 rows, through one target column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edlib_amd {

// One column of Myers' bit-vector recurrence over the NWD words of a lane (reference calculateBlock, edlib.cpp:422-460, on
// 32-row words, the horizontal delta carried from word to word).  The top row's delta is 0 for HW, +1 for NW / SHW.
// `rows` is the Peq row of the column's symbol, word d at rows[d * stride].
// Returns nothing; `score` follows the bottom row m - 1 (bit sh of the last word).
template <int NWD, int MODE>
__device__ __forceinline__ void cross_column(const uint32_t* __restrict__ rows, int stride, uint32_t (&Pv)[NWD],
                                             uint32_t (&Mv)[NWD], const int sh, int& score)
{
    typedef uint32_t u32;
    u32 hinPos = MODE == 2 ? 0u : 1u, hinNeg = 0u;
#pragma unroll
    for (int d = 0; d < NWD; ++d) {
        u32 eq = rows[d * stride];
        const u32 xv = eq | Mv[d];
        eq |= hinNeg;
        const u32 pv = Pv[d];
        const u32 xh = (((eq & pv) + pv) ^ pv) | eq;
        u32 ph = Mv[d] | ~(xh | pv);
        u32 mh = pv & xh;
        if (d == NWD - 1) score += (int)((ph >> sh) & 1u) - (int)((mh >> sh) & 1u);
        const u32 hop = ph >> 31, hom = mh >> 31;
        ph = (ph << 1) | hinPos;
        mh = (mh << 1) | hinNeg;
        Pv[d] = mh | ~(xv | ph);
        Mv[d] = ph & xv;
        hinPos = hop; hinNeg = hom;
    }
}

}  // namespace edlib_amd
