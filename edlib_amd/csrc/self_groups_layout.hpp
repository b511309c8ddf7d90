// self_groups_layout.hpp -- the host layout of a grouped self batch (DESIGN.md §4h "Grouped self batches") and the lane
// predicate its kernel shares with it.  Plain C++17 without HIP: engine_self.hip (initSelfGrouped) and the kernel
// (cross_scan.hpp, GROUPS) include it, and tests/self_groups_host.cpp runs it on the host.
// The kernel's sequences are sorted by (group, length, index); a sequence's place there is its rank, end[r] is one past the
// last rank of r's group.  Inside a group the rank rises with the length, so the lower rank of a pair is still its shorter
// sequence and still the rows.  Slot s of word group w holds the s-th rank (ascending) whose sequence has w words.  A work
// item is a query tile against a run of target tiles, as in an ungrouped self batch; which lanes of it hold a wanted pair
// is self_groups_lane().  The host's share is one sort and linear passes (a binary search per run of slots).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDLIB_AMD_HD __host__ __device__
#else
#define EDLIB_AMD_HD
#endif

namespace edlib_amd {

// Lane `lane` (0..63) of a wave on target tile `tt` of a word group whose tiles hold qt slots: the slot of its tile it
// takes (`slotInTile`, so slot = tile * qt + slotInTile), its target rank `ts`, and whether the pair is wanted.  rank and
// end are qrank[slot] and qend[slot] of that slot (-1 on padding, which is never live); end <= numSorted.
EDLIB_AMD_HD inline bool self_groups_lane(int qt, int lane, int tt, int rank, int end, int numSorted, int& slotInTile, int& ts)
{
    slotInTile = lane & (qt - 1);
    ts = tt * (64 / qt) + lane / qt;
    return ts < numSorted && ts > rank && ts < end;
}

struct SelfGroupsRange { int tile, first, last; };        // the target tiles [first, last] a run of slots of `tile` wants

struct SelfGroupsWordGroup {
    int words = 0, qt = 64, tiles = 0;
    long long wordSteps = 0, trips = 0;
    std::vector<int> perm, rank, end;       // [tiles * qt]: sequence index, rank and end[rank] of every slot, -1 on padding
    std::vector<int> items;                 // triples (query tile, first target tile, trips)
    std::vector<SelfGroupsRange> runs;      // (keepRuns) the range of every run of slots that has one, by tile
};

struct SelfGroupsLayout {
    std::vector<int> order, tlen, end;      // per rank: the sequence, its length, one past the last rank of its group
    std::vector<SelfGroupsWordGroup> wordGroups;          // those with at least one item
    long long wordSteps = 0, wanted = 0, trips = 0;       // wanted: pairs inside the length window; trips: of all items
};

// Tile width of a word group of `cnt` slots whose slot wants `partners` target ranks on average.  A tile's runs start at
// its own slots, so its trips cover about qt + partners ranks, 64 / qt a trip: the lanes that costs decide, and among the
// widths within 1 / 64 of the fewest the widest tile wins (fewer Peq stagings; one large group keeps the 64 of an
// ungrouped self batch).  Only lane occupancy depends on it.
inline int self_groups_choose_qt(long long cnt, double partners)
{
    const long long p = (long long)partners + (partners > (double)(long long)partners ? 1 : 0);
    long long lanes[7], fewest = -1;
    for (int i = 0; i < 7; ++i) {
        const long long qt = 64 >> i, tpt = 64 / qt;
        lanes[i] = ((cnt + qt - 1) / qt) * 64 * ((qt + p + tpt - 1) / tpt);
        if (fewest < 0 || lanes[i] < fewest) fewest = lanes[i];
    }
    for (int i = 0; i < 7; ++i)
        if (lanes[i] <= fewest + fewest / 64) return 64 >> i;
    return 1;
}

// seqs: the sequences the kernel takes (1..32 * maxWords bases each), in any order; group(i) and len(i) their label and
// length.  k >= 0: the length window.
template <typename GroupOf, typename LenOf>
inline SelfGroupsLayout self_groups_layout(std::vector<int> seqs, GroupOf group, LenOf len, int k, int maxWords,
                                           bool keepRuns = false)
{
    SelfGroupsLayout L;
    std::sort(seqs.begin(), seqs.end(), [&](int a, int b) {
        if (group(a) != group(b)) return group(a) < group(b);
        if (len(a) != len(b)) return len(a) < len(b);
        return a < b;
    });
    const int n = (int)seqs.size();
    L.order = std::move(seqs);
    L.tlen.resize(n); L.end.resize(n);
    std::vector<long long> colsBelow((size_t)n + 1, 0);
    for (int r = 0; r < n; ++r) { L.tlen[r] = len(L.order[r]); colsBelow[r + 1] = colsBelow[r] + L.tlen[r]; }
    for (int r0 = 0; r0 < n;) {
        int r1 = r0;
        while (r1 < n && group(L.order[r1]) == group(L.order[r0])) ++r1;
        for (int r = r0; r < r1; ++r) L.end[r] = r1;
        r0 = r1;
    }
    // one past the last rank of r's group inside the length window of a row of length m, not below `from` (a rank of that group)
    auto windowEnd = [&](int from, int m) -> int {
        return (int)(std::upper_bound(L.tlen.begin() + from, L.tlen.begin() + L.end[from], (long long)m + k) - L.tlen.begin());
    };
    // per rank what its row scans: the ranks (r, hi(r)), hi rising with r inside a group
    std::vector<long long> partners((size_t)maxWords + 1, 0), steps((size_t)maxWords + 1, 0);
    std::vector<int> count((size_t)maxWords + 1, 0);
    for (int r = 0, hi = 0; r < n; ++r) {
        if (hi < r + 1) hi = r + 1;
        while (hi < L.end[r] && (long long)L.tlen[hi] <= (long long)L.tlen[r] + k) ++hi;
        if (hi > L.end[r]) hi = L.end[r];                    // (the next group's first rank starts above its own r + 1)
        const int w = (L.tlen[r] + 31) / 32;
        ++count[w];
        partners[w] += hi - (r + 1);
        steps[w] += (long long)w * (colsBelow[hi] - colsBelow[r + 1]);
        if (r + 1 < n && L.end[r + 1] != L.end[r]) hi = 0;
    }
    for (int w = 1; w <= maxWords; ++w) {
        if (partners[w] == 0) continue;                      // no row of this word count has a partner: no item
        SelfGroupsWordGroup g;
        g.words = w;
        g.wordSteps = steps[w];
        g.qt = self_groups_choose_qt(count[w], (double)partners[w] / (double)count[w]);
        g.tiles = (count[w] + g.qt - 1) / g.qt;
        const int tpt = 64 / g.qt;
        g.perm.assign((size_t)g.tiles * g.qt, -1); g.rank = g.perm; g.end = g.perm;
        int s = 0;
        for (int r = 0; r < n; ++r)
            if ((L.tlen[r] + 31) / 32 == w) { g.perm[s] = L.order[r]; g.rank[s] = r; g.end[s] = L.end[r]; ++s; }
        // per tile: every maximal run of slots that share a group wants the ranks (its lowest rank, hi), hi the end of the
        // length window of its longest query (its last slot) inside the group; ranges that overlap or touch are merged
        std::vector<SelfGroupsRange> merged;
        std::vector<std::pair<int, int>> ranges;
        for (int t = 0; t < g.tiles; ++t) {
            ranges.clear();
            const int s1 = std::min(count[w], (t + 1) * g.qt);
            for (int a = t * g.qt; a < s1;) {
                int b = a;
                while (b < s1 && g.end[b] == g.end[a]) ++b;
                const int lo = g.rank[a] + 1, hi = windowEnd(g.rank[b - 1], L.tlen[g.rank[b - 1]]);
                if (hi > lo) {
                    ranges.emplace_back(lo / tpt, (hi - 1) / tpt);
                    if (keepRuns) g.runs.push_back({t, lo / tpt, (hi - 1) / tpt});
                }
                a = b;
            }
            std::sort(ranges.begin(), ranges.end());
            for (size_t i = 0; i < ranges.size(); ++i) {
                if (!merged.empty() && merged.back().tile == t && ranges[i].first <= merged.back().last + 1)
                    merged.back().last = std::max(merged.back().last, ranges[i].second);
                else merged.push_back({t, ranges[i].first, ranges[i].second});
            }
        }
        for (const SelfGroupsRange& m : merged) g.trips += m.last - m.first + 1;
        // work items of about equal trip counts, about 8,192 of them per launch: a range is cut into equal parts of at
        // most `chunk` trips, never under 16 trips unless the range is shorter (the rule of an ungrouped self batch)
        const long long chunk = std::max(16LL, (g.trips + 8191) / 8192);
        for (const SelfGroupsRange& m : merged) {
            const long long trips = m.last - m.first + 1;
            const long long parts = std::max(1LL, std::min((trips + chunk - 1) / chunk, trips / 16));
            for (long long p = 0; p < parts; ++p) {
                const long long a = trips * p / parts, b = trips * (p + 1) / parts;
                g.items.push_back(m.tile); g.items.push_back(m.first + (int)a); g.items.push_back((int)(b - a));
            }
        }
        L.wordSteps += g.wordSteps; L.wanted += partners[w]; L.trips += g.trips;
        L.wordGroups.push_back(std::move(g));
    }
    return L;
}

}  // namespace edlib_amd
