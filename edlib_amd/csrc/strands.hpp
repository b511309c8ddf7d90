// strands.hpp -- both-strand read batches: a read and its reverse complement are the units 2i and 2i + 1
// of one batch, mates sit in the slots s and s ^ 1 of their word-count group, and one of them is reported.
#pragma once
#include "common.hpp"

namespace edlib_amd {

// The complement of a nucleotide code (IUPAC, both cases; U / u -> A / a); every other byte is its own.
__host__ __device__ inline uint8_t complement_byte(uint8_t b)
{
    const bool lower = b >= 'a' && b <= 'z';
    uint8_t r;
    switch (lower ? (uint8_t)(b - 32) : b) {
        case 'A': r = 'T'; break;  case 'T': r = 'A'; break;  case 'U': r = 'A'; break;
        case 'C': r = 'G'; break;  case 'G': r = 'C'; break;
        case 'R': r = 'Y'; break;  case 'Y': r = 'R'; break;
        case 'K': r = 'M'; break;  case 'M': r = 'K'; break;
        case 'B': r = 'V'; break;  case 'V': r = 'B'; break;
        case 'D': r = 'H'; break;  case 'H': r = 'D'; break;
        default: return b;                                          // S, W, N and everything that is no code
    }
    return lower ? (uint8_t)(r + 32) : r;
}

// What a mate pair reports (the table of edlib_amd.h): bit 0 the winning strand, kStrandBoth: the other strand reaches the
// same distance, kStrandNone: neither strand has an alignment within k (the forward record, distance -1, is reported).
constexpr int kStrandReverse = 1, kStrandBoth = 2, kStrandNone = 4;
__host__ __device__ inline int resolve_strands(int dFwd, int dRev)
{
    if (dFwd >= 0 && (dRev < 0 || dFwd <= dRev)) return dRev == dFwd ? kStrandBoth : 0;
    return dRev >= 0 ? kStrandReverse : kStrandNone;
}

// The query pool of a both-strand batch, made from the caller's pool `in` (numReads reads back to back from offset 0):
// read i goes to off2[2 i], its reverse complement to off2[2 i + 1] = off2[2 i] + its length; off2[2 i] is twice the read's
// offset in `in`.  A wave per read.
hipError_t launch_strand_pool(const uint8_t* in, const long long* off2, int numReads, uint8_t* out, hipStream_t stream);

// The same for a batch that holds the caller's offsets: `queries` are the nq queries back to back, off[0 .. nq] their
// offsets from 0.  The bytes go up as they are, d_off gets the 2 nq + 1 offsets described above, d_pool the pool made by
// launch_strand_pool, and the stream is waited for.  0, or 1 with the error set.
int make_strand_pool(const char* queries, const long long* off, int nq, DevBuf<uint8_t>& d_pool, DevBuf<long long>& d_off,
                     hipStream_t stream);

// win[p] of the mate pair in the slots 2 p, 2 p + 1 of a read group, from the merged per-slot records (best, total).
// mode 0: NW (the score is the distance unless it exceeds k), else SHW / HW (a slot has an alignment iff total > 0).
hipError_t launch_resolve_strands(const int* perm, const int* best, const int* total, int nslots, int mode, int k, int* win,
                                  hipStream_t stream);

// slot -> read order of the WINNING slots of one group: what flat_results.hip reads per unit, and the two strand bytes.
// Read = perm[slot] >> 1.
hipError_t launch_gather_group_strands(const int* perm, int nslots, const int* win, const int* best, const int* total,
                                       const int* qlen, const int* extra, const int* pos, int posCap, int* uScore, int* uCount,
                                       int* uQlen, int* uAlpha, int* uPos, uint8_t* uStrand, uint8_t* uBoth, hipStream_t stream);

}  // namespace edlib_amd
