// segment_plan.hpp -- how a scan launch over one shared target is cut into segments.  Plain C++ with no
// device code: the engine includes it, and tests/tapered_plan_host.cpp compiles it for the host alone.
#pragma once
#include <algorithm>
#include <vector>

namespace edlib_amd {

struct Segment { int start, cols; };     // columns [start, start + cols) of the target

constexpr int kMaxSegments = 65535;      // gridDim.y

inline int seg_roundup16(long long x) { return (int)((x + 15) / 16 * 16); }

// Uniform segmentation of a launch over `nlanes` lanes: enough waves to fill the chip, segments >= minSegCols columns and,
// with a warm-up, at least four warm-ups long.  hw: the mode cuts at all (HW).
inline void plan_segments_uniform(int nlanes, int T, bool hw, int warmFull, long long wantWaves, int minSegCols,
                                  int& S, int& segLen, int& warm)
{
    S = 1; segLen = seg_roundup16(T); warm = 0;
    if (!hw) return;
    const long long nrblk = ((long long)nlanes + 63) / 64;
    long long want = (wantWaves + nrblk - 1) / nrblk;
    want = std::max(1LL, std::min<long long>(want, std::min(kMaxSegments, std::max(1, T / minSegCols))));   // gridDim.y limit
    if (warmFull > 0) want = std::max(1LL, std::min<long long>(want, std::max<long long>(1, T / (4LL * warmFull))));   // >= four warm-ups per segment
    segLen = seg_roundup16((T + want - 1) / want);
    S = (T + segLen - 1) / segLen;
    warm = warmFull;
}

// the table of the uniform plan: segments of Lmax columns, the last one ragged
inline std::vector<Segment> uniform_segment_table(int T, int Lmax)
{
    std::vector<Segment> t;
    for (long long c = 0; c < T; c += Lmax) t.push_back({(int)c, (int)std::min<long long>(Lmax, T - c)});
    return t;
}

// Tapered segmentation of one launch of gridX workgroups per segment, of which `resident` fit on the device at once.
// A launch of uniform segments ends ragged: the workgroups drift apart, and once the queue is empty every workgroup that
// finishes leaves its slot to nothing, for as long as the longest one still has to go -- up to a whole segment.  Here every
// segment is a fixed share of what is left when it is cut: remaining / (2 R) columns, R = resident / gridX the rows of
// segments that are resident together, so that the work still queued behind a row is always about two rounds of rows like
// it and the last rows are short.  Lengths are multiples of 16 (no group of four or eight columns straddles a restart) between
// minCols (four warm-ups: a shorter segment pays more warm-up than that per column of its own) and Lmax (the uniform length);
// the last segment takes the ragged rest.  Ascending in the target: the short segments are the END of the target, the
// highest blockIdx.y.  Nothing depends on the order in which the device starts them; it only shortens the drain.
// Where the taper cannot pay -- Lmax <= minCols, or fewer than two rounds of workgroups -- the table is the uniform plan's.
inline std::vector<Segment> plan_segments_tapered(int T, int gridX, int resident, int warm, int Lmax)
{
    Lmax = std::max(16, Lmax / 16 * 16);
    int minCols = std::max(16, seg_roundup16(4LL * warm));
    // every segment but the last is >= minCols: at most kMaxSegments of them
    minCols = std::max(minCols, seg_roundup16(((long long)T + kMaxSegments - 2) / (kMaxSegments - 1)));
    const long long uniformS = ((long long)T + Lmax - 1) / Lmax;
    if (T <= 0 || gridX <= 0 || resident <= 0 || Lmax <= minCols || uniformS * gridX < 2LL * resident)
        return uniform_segment_table(T, Lmax);
    std::vector<Segment> t;
    long long c = 0;
    while (c < T) {
        const long long rem = T - c;
        long long len = rem * gridX / (2LL * resident) / 16 * 16;          // remaining / (2 R), down to a multiple of 16
        len = std::max<long long>(minCols, std::min<long long>(Lmax, len));
        if (len > rem) len = rem;                                           // the ragged last
        t.push_back({(int)c, (int)len});
        c += len;
    }
    return t;
}

}  // namespace edlib_amd
