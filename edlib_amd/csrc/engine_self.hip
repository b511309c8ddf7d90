// engine_self.hip -- the self mode of the cross engine (DESIGN.md §4h "Self batches"): one set against itself, NW
// distances, every unordered pair once.  Create puts the sequences the kernel takes into the order (length, index) -- a
// sequence's place there is its rank --, packs them once as the targets, makes the word groups (runs of that order) the
// query slots, and cuts every query tile's range of wanted target tiles into work items of about equal trip counts.  A
// Run builds the Peq rows, scans the items of every group, lets the internal pair batch take the pairs outside the
// kernel's envelope, and reduces the nearest other sequence of each on the device.  The pack, the Peq build, the hit
// list and its finish are the cross batch's own (engine_cross.hip, hit_list.hpp, cross_hits.hip).
// A both-strand self batch reports for every pair i < j the better of NW(seq i, seq j) and NW(revcomp(seq i), seq j).  The
// kernel reverse-complements the row sequence, the shorter one, which is the same only under the complement condition
// below; a set that fails it goes through the pair batch whole, in index order.
#include "engine_lanes.hpp"
#include "self_groups_layout.hpp"

#include <algorithm>
#include <cstring>
#include <utility>

namespace edlib_amd {

typedef unsigned long long u64;

// The complement condition of a both-strand self batch: Eq(c(x), y) <=> Eq(x, c(y)) for all bytes x, y of the set, with
// c = complement_byte and Eq the batch's match relation.  Then NW(revcomp(a), b) == NW(revcomp(b), a), so the kernel may
// reverse-complement whichever sequence of a pair it has in the rows.
static bool complement_symmetric(const Tables& tab)
{
    auto eq = [&](int x, int y) { return tab.eq8.empty() ? x == y : tab.eq8[(size_t)x * 256 + y] != 0; };
    for (int s = 0; s < tab.sigmaT; ++s)
        for (int t = 0; t < tab.sigmaT; ++t) {
            const int x = tab.idToByte[s], y = tab.idToByte[t];
            if (eq(complement_byte((uint8_t)x), y) != eq(x, complement_byte((uint8_t)y))) return false;
        }
    return true;
}

int CrossBatch::initSelf(const char* seqs, const long long* offIn, int n, EdlibAlignConfig cfg, int device, bool hits,
                         bool strands)
{
    if (cfg.task != EDLIB_TASK_DISTANCE) {
        set_error("self batches compute distances only (EDLIB_TASK_DISTANCE): align the chosen pairs with a pair batch "
                  "for locations or paths");
        return 1;
    }
    if (cfg.mode == EDLIB_MODE_HW || cfg.mode == EDLIB_MODE_SHW) {
        set_error("self batches are global (EDLIB_MODE_NW): %s distances are not symmetric, pass the set as queries and "
                  "as targets of a cross batch", cfg.mode == EDLIB_MODE_HW ? "HW" : "SHW");
        return 1;
    }
    if (cfg.mode != EDLIB_MODE_NW) { set_error("unknown mode"); return 1; }
    if (hits && cfg.k < 0) {
        set_error("hit-list self batches need config.k >= 0 (every pair is a hit at k = %d: use edlibAmdBatchCreateSelf "
                  "for the condensed distances)", cfg.k);
        return 1;
    }
    if (n < 0 || (n > 0 && !offIn)) { set_error("bad batch shape"); return 1; }
    if (strands && n > 0x3fffffff) { set_error("bad both-strand batch shape"); return 1; }
    std::vector<long long> off;
    if (copy_offsets(offIn, n, "sequence", off) || check_device(device)) return 1;      // (the offsets first: edlib_amd.h)
    keep_config(cfg, cfg_, eqs_);
    device_ = device; nq_ = nt_ = n; hits_ = hits; strands_ = strands; self_ = true;
    const long long base = off[0], bytes = off[n] - base;
    auto len = [&](int i) { return (int)(off[i + 1] - off[i]); };
    const long long numPairs = (long long)n * (n - 1) / 2;
    cells_ = (size_t)std::max(numPairs, 0LL);
    stats = EdlibAmdBatchStats{};
    {   // sum over i < j of m_i m_j = ((sum m)^2 - sum m^2) / 2
        unsigned __int128 sq = 0;
        for (int i = 0; i < n; ++i) sq += (unsigned __int128)len(i) * (unsigned __int128)len(i);
        stats.cells = (long long)((((unsigned __int128)bytes * (unsigned __int128)bytes) - sq) / 2) * (strands ? 2 : 1);
    }
    auto key = [](int i, int j) { return ((u64)(uint32_t)std::min(i, j) << 32) | (uint32_t)std::max(i, j); };
    auto inWindow = [&](int a, int b) {
        const long long d = (long long)len(a) - len(b);
        return cfg.k < 0 || (d < 0 ? -d : d) <= cfg.k;
    };

    build_tables(tab_, reinterpret_cast<const uint8_t*>(seqs) + base, bytes, eqs_.data(), (int)eqs_.size());
    // (both strands: a set that fails the complement condition is the pair batch's whole, like one of too many symbols)
    const bool wide = tab_.sigmaT > kCrossMaxSyms || (strands && !complement_symmetric(tab_));
    syms_ = peq_syms(tab_.sigmaT);
    // the kernel's sequences in the order (length, index); the empty ones are answered here, the others by the pair batch
    std::vector<int> inK, empties, outK;
    for (int i = 0; i < n; ++i) {
        if (len(i) == 0) empties.push_back(i);
        else if (!wide && len(i) <= 32 * kCrossMaxQueryWords) inK.push_back(i);
        else outK.push_back(i);
    }
    std::stable_sort(inK.begin(), inK.end(), [&](int a, int b) { return len(a) < len(b); });

    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    if (openStream()) return 1;
    EDLIB_AMD_HIP(d_near_.alloc(3 * (size_t)n));
    if (strands_) {
        EDLIB_AMD_HIP(d_sbest_.alloc(3 * (size_t)std::max(n, 1)));
        if (!hits_) EDLIB_AMD_HIP(d_smat_.alloc(std::max<size_t>(cells_, 1)));
    }
    if (!hits_) EDLIB_AMD_HIP(d_mat_.alloc(std::max<size_t>(cells_, 1)));
    else {
        EDLIB_AMD_HIP(d_best_.alloc(6 * (size_t)n));
        EDLIB_AMD_HIP(d_bkey_.alloc(4 * (size_t)n));
        if (sizeHitList(std::max<long long>(1LL << 20, 2LL * n))) return 1;
    }

    // (what a pair batch that gathers from this one is checked against: CrossBatch::gatherSource)
    tlenHost_.resize((size_t)n);
    for (int i = 0; i < n; ++i) tlenHost_[i] = len(i);
    inPack_.assign((size_t)n, 0);

    // ---- the kernel's share
    if (inK.size() >= 2) {
        numSorted_ = (int)inK.size();
        for (int i : inK) inPack_[i] = 1;
        std::vector<long long> colsBelow(numSorted_ + 1, 0);
        std::vector<int> tl(numSorted_);
        for (int r = 0; r < numSorted_; ++r) {
            tl[r] = len(inK[r]);
            sortedCols_ += tl[r];
            colsBelow[r + 1] = sortedCols_;
        }
        // one past the last rank inside the length window of a row of length m (rows are the shorter sequence)
        auto windowEnd = [&](int m) -> int {
            if (cfg.k < 0) return numSorted_;
            return (int)(std::upper_bound(tl.begin(), tl.end(), (long long)m + cfg.k) - tl.begin());
        };
        // the pool goes up once: the pack reads it as the targets, the Peq build as the queries
        if (!strands_) {
            if (uploadQueries(seqs, off, false) || packTargets(d_qpool_.p, d_qoff_.p, inK, tl)) return 1;
        } else {
            // sequence i and its reverse complement are the entries 2 i and 2 i + 1 of the pool: the targets are packed
            // from the forward copies, and d_tperm_ names sequences again behind the pack
            std::vector<int> fwd(inK);
            for (int& i : fwd) i *= 2;
            if (uploadQueries(seqs, off, true) || packTargets(d_qpool_.p, d_qoff_.p, fwd, tl)) return 1;
            EDLIB_AMD_HIP(hipMemcpy(d_tperm_.p, inK.data(), inK.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        EDLIB_AMD_HIP(d_tlen_.alloc(numSorted_));
        EDLIB_AMD_HIP(hipMemcpy(d_tlen_.p, tl.data(), numSorted_ * sizeof(int), hipMemcpyHostToDevice));
        // a word group is a run of ranks [r0, r1): its slot s holds rank r0 + s, so the rank rises with the slot
        // (both strands: the slots 2 s and 2 s + 1 hold rank r0 + s and its reverse complement, `per` = 2 slots a rank)
        const int per = strands_ ? 2 : 1;
        for (int r0 = 0; r0 < numSorted_;) {
            const int w = (tl[r0] + 31) / 32;
            int r1 = r0;
            while (r1 < numSorted_ && (tl[r1] + 31) / 32 == w) ++r1;
            const int cnt = r1 - r0;
            std::unique_ptr<Group> g(new Group);
            g->words = w;
            g->qt = choose_qt((long long)per * cnt, numSorted_, per);
            const int spt = g->qt / per;                                   // sequences of a query tile
            g->tiles = (cnt + spt - 1) / spt;
            const int tpt = 64 / g->qt;
            std::vector<int> perm((size_t)g->tiles * g->qt, -1), rank(perm.size(), -1);      // whole tiles
            for (int s = 0; s < cnt; ++s) {
                for (int st = 0; st < per; ++st) { perm[per * s + st] = per * inK[r0 + s] + st; rank[per * s + st] = r0 + s; }
                g->wordSteps += (long long)per * w * (colsBelow[windowEnd(tl[r0 + s])] - colsBelow[r0 + s + 1]);
            }
            if (strands_) {
                // what the kernel's lane exchange rests on: mates in the slots s and s ^ 1, padding in pairs, an even tile
                bool ok = !(g->qt & 1) && !(perm.size() & 1);
                for (size_t sl = 0; ok && sl < perm.size(); sl += 2)
                    ok = perm[sl] < 0 ? perm[sl + 1] < 0
                                      : (!(perm[sl] & 1) && perm[sl + 1] == perm[sl] + 1 && rank[sl + 1] == rank[sl]);
                if (!ok) { set_error("both strands: mates are not in adjacent slots"); return 1; }
            }
            // per query tile the target tiles that hold a wanted cell inside the length window: from the tile of the rank
            // behind the tile's lowest to the tile of the last rank within k of the tile's longest query
            std::vector<int> first(g->tiles), trips(g->tiles);
            long long allTrips = 0;
            for (int t = 0; t < g->tiles; ++t) {
                const int lo = r0 + t * spt + 1, hi = windowEnd(tl[r0 + std::min(cnt, (t + 1) * spt) - 1]);
                first[t] = lo / tpt;
                trips[t] = hi > lo ? (hi - 1) / tpt - first[t] + 1 : 0;
                allTrips += trips[t];
            }
            // work items of about equal trip counts, about 8,192 of them per launch (256 CUs; the cross launch's aim): a
            // range is cut into equal parts of at most `chunk` trips, never under 16 trips unless the range is shorter, so
            // the Peq staging of an item stays amortised
            const long long chunk = std::max(16LL, (allTrips + 8191) / 8192);
            std::vector<int> items;
            for (int t = 0; t < g->tiles; ++t) {
                if (trips[t] == 0) continue;
                const long long parts = std::max(1LL, std::min((trips[t] + chunk - 1) / chunk, (long long)trips[t] / 16));
                for (long long p = 0; p < parts; ++p) {
                    const long long a = trips[t] * p / parts, b = trips[t] * (p + 1) / parts;
                    items.push_back(t); items.push_back(first[t] + (int)a); items.push_back((int)(b - a));
                }
            }
            g->numItems = (int)(items.size() / 3);
            if (allocGroup(*g, perm)) return 1;
            EDLIB_AMD_HIP(g->d_rank.alloc(g->slots)); EDLIB_AMD_HIP(g->d_items.alloc(std::max<size_t>(items.size(), 3)));
            EDLIB_AMD_HIP(hipMemcpy(g->d_rank.p, rank.data(), g->slots * sizeof(int), hipMemcpyHostToDevice));
            if (!items.empty())
                EDLIB_AMD_HIP(hipMemcpy(g->d_items.p, items.data(), items.size() * sizeof(int), hipMemcpyHostToDevice));
            groups_.push_back(std::move(g));
            r0 = r1;
        }
    }

    // ---- the pairs answered off the kernel: those with an empty sequence here, the rest by one pair batch
    for (int e : empties)
        for (int x = 0; x < n; ++x) {
            if (x == e || (len(x) == 0 && x < e)) continue;          // two empty sequences: once
            selfOther_.push_back(key(e, x));
            selfEmptyVal_.push_back(len(x));
        }
    {
        PairPool pool;
        const int per = strands_ ? 2 : 1;
        long long np = 0;
        auto add = [&](int i, int j) {                                // i < j, both with bases
            if (!inWindow(i, j)) return;
            if ((np += per) > 0x7fffffffLL) return;
            // (both strands: the pairs 2c and 2c + 1 of pair c, the second with the lower index's reverse complement)
            for (int st = 0; st < per; ++st) pool.add(seqs + off[i], len(i), st != 0, seqs + off[j], len(j));
            selfOther_.push_back(key(i, j));
        };
        std::vector<char> isOut(n, 0);
        for (int i : outK) isOut[i] = 1;
        for (int i : outK)
            for (int x = 0; x < n && np <= 0x7fffffffLL; ++x) {
                if (x == i || len(x) == 0 || (isOut[x] && x < i)) continue;   // two such sequences: once
                add(std::min(i, x), std::max(i, x));
            }
        if (np > 0x7fffffffLL) {
            set_error("self batch: too many pairs outside the kernel's envelope (more than 2^31 - 1%s): sequences above %d "
                      "bases or a set with more than %d symbols%s", strands_ ? ", both strands counted" : "",
                      32 * kCrossMaxQueryWords, kCrossMaxSyms,
                      strands_ ? ", or one whose equalities are not closed under complement" : "");
            return 1;
        }
        if (np > 0) {
            longPairs_.reset(new Batch);
            if (pool.init(*longPairs_, cfg_, device)) return 1;
        }
    }
    otherCells_ = (long long)selfOther_.size();
    if (otherCells_ > 0) {
        EDLIB_AMD_HIP(h_vals_.alloc((size_t)otherCells_ * sizeof(int)));
        std::copy(selfEmptyVal_.begin(), selfEmptyVal_.end(), reinterpret_cast<int*>(h_vals_.p));
        if (strands_) {
            // an empty sequence is its own reverse complement: both strands reach the other's length
            EDLIB_AMD_HIP(h_svals_.alloc((size_t)otherCells_));
            std::fill(h_svals_.p, h_svals_.p + selfEmptyVal_.size(), (uint8_t)kStrandBoth);
            if (!hits_) EDLIB_AMD_HIP(d_svals_.alloc((size_t)otherCells_));
        }
        if (!hits_) {
            std::vector<long long> cellIdx((size_t)otherCells_);
            for (size_t c = 0; c < cellIdx.size(); ++c) {
                const long long i = (long long)(selfOther_[c] >> 32), j = (long long)(uint32_t)selfOther_[c];
                cellIdx[c] = (long long)n * i - i * (i + 1) / 2 + (j - i - 1);
            }
            EDLIB_AMD_HIP(d_cells_.alloc((size_t)otherCells_)); EDLIB_AMD_HIP(d_vals_.alloc((size_t)otherCells_));
            EDLIB_AMD_HIP(hipMemcpy(d_cells_.p, cellIdx.data(), (size_t)otherCells_ * sizeof(long long), hipMemcpyHostToDevice));
        }
    }
    return 0;
}

// A grouped self batch: the checks and the routes of a hit-list self batch, every route restricted to the pairs inside a
// group.  The kernel's order, word groups and work items are self_groups_layout.hpp's; the host's share is that sort, a
// sort of the indices by (group, index) for the other routes, and linear passes.
int CrossBatch::initSelfGrouped(const char* seqs, const long long* offIn, int n, const int* groups, EdlibAlignConfig cfg,
                                int device)
{
    if (!groups && n > 0) {
        set_error("grouped self batch: groups is NULL (one int label per sequence; a set without groups is "
                  "edlibAmdBatchCreateSelfHits)");
        return 1;
    }
    if (cfg.task != EDLIB_TASK_DISTANCE) {
        set_error("self batches compute distances only (EDLIB_TASK_DISTANCE): align the chosen pairs with a pair batch "
                  "for locations or paths");
        return 1;
    }
    if (cfg.mode == EDLIB_MODE_HW || cfg.mode == EDLIB_MODE_SHW) {
        set_error("self batches are global (EDLIB_MODE_NW): %s distances are not symmetric, pass the set as queries and "
                  "as targets of a cross batch", cfg.mode == EDLIB_MODE_HW ? "HW" : "SHW");
        return 1;
    }
    if (cfg.mode != EDLIB_MODE_NW) { set_error("unknown mode"); return 1; }
    if (cfg.k < 0) {
        set_error("grouped self batches are hit lists and need config.k >= 0 (got %d; there is no dense grouped form: the "
                  "condensed vector has no meaning across groups -- pass a k that bounds the distances wanted)", cfg.k);
        return 1;
    }
    if (n < 0 || (n > 0 && !offIn)) { set_error("bad batch shape"); return 1; }
    std::vector<long long> off;
    if (copy_offsets(offIn, n, "sequence", off) || check_device(device)) return 1;
    keep_config(cfg, cfg_, eqs_);
    device_ = device; nq_ = nt_ = n; hits_ = true; strands_ = false; self_ = true; grouped_ = true;
    const long long base = off[0], bytes = off[n] - base;
    auto len = [&](int i) { return (int)(off[i + 1] - off[i]); };
    auto key = [](int i, int j) { return ((u64)(uint32_t)std::min(i, j) << 32) | (uint32_t)std::max(i, j); };
    auto inWindow = [&](int a, int b) {
        const long long d = (long long)len(a) - len(b);
        return (d < 0 ? -d : d) <= cfg.k;
    };
    // the members of every group, ascending: byGroup[memberOff[g] .. memberOff[g + 1]), groupOf[i] = g
    std::vector<int> byGroup(n), groupOf(n), memberOff(1, 0);
    for (int i = 0; i < n; ++i) byGroup[i] = i;
    std::sort(byGroup.begin(), byGroup.end(), [&](int a, int b) { return groups[a] != groups[b] ? groups[a] < groups[b] : a < b; });
    stats = EdlibAmdBatchStats{};
    {   // per group: its pairs, and the sum over i < j of m_i m_j = ((sum m)^2 - sum m^2) / 2
        long long pairs = 0;
        unsigned __int128 cells = 0;
        for (int a = 0; a < n;) {
            int b = a;
            unsigned __int128 sum = 0, sq = 0;
            for (; b < n && groups[byGroup[b]] == groups[byGroup[a]]; ++b) {
                groupOf[byGroup[b]] = (int)memberOff.size() - 1;
                sum += (unsigned __int128)len(byGroup[b]);
                sq += (unsigned __int128)len(byGroup[b]) * (unsigned __int128)len(byGroup[b]);
            }
            pairs += (long long)(b - a) * (b - a - 1) / 2;
            cells += (sum * sum - sq) / 2;
            memberOff.push_back(b);
            a = b;
        }
        cells_ = (size_t)pairs;
        stats.cells = (long long)cells;
    }

    build_tables(tab_, reinterpret_cast<const uint8_t*>(seqs) + base, bytes, eqs_.data(), (int)eqs_.size());
    const bool wide = tab_.sigmaT > kCrossMaxSyms;
    syms_ = peq_syms(tab_.sigmaT);
    std::vector<int> inK, empties, outK;
    for (int i = 0; i < n; ++i) {
        if (len(i) == 0) empties.push_back(i);
        else if (!wide && len(i) <= 32 * kCrossMaxQueryWords) inK.push_back(i);
        else outK.push_back(i);
    }

    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    if (openStream()) return 1;
    EDLIB_AMD_HIP(d_near_.alloc(3 * (size_t)n));
    EDLIB_AMD_HIP(d_best_.alloc(6 * (size_t)n));
    EDLIB_AMD_HIP(d_bkey_.alloc(4 * (size_t)n));
    if (sizeHitList(std::max<long long>(1LL << 20, 2LL * n))) return 1;

    // (what a pair batch that gathers from this one is checked against: CrossBatch::gatherSource)
    tlenHost_.resize((size_t)n);
    for (int i = 0; i < n; ++i) tlenHost_[i] = len(i);
    inPack_.assign((size_t)n, 0);

    // ---- the kernel's share
    if (inK.size() >= 2) {
        SelfGroupsLayout lay = self_groups_layout(std::move(inK), [&](int i) { return groups[i]; }, len, cfg.k,
                                                  kCrossMaxQueryWords);
        numSorted_ = (int)lay.order.size();
        for (int i : lay.order) inPack_[i] = 1;
        for (int m : lay.tlen) sortedCols_ += m;
        // the pool goes up once: the pack reads it as the targets, the Peq build as the queries
        if (uploadQueries(seqs, off, false) || packTargets(d_qpool_.p, d_qoff_.p, lay.order, lay.tlen)) return 1;
        EDLIB_AMD_HIP(d_tlen_.alloc(numSorted_));
        EDLIB_AMD_HIP(hipMemcpy(d_tlen_.p, lay.tlen.data(), numSorted_ * sizeof(int), hipMemcpyHostToDevice));
        for (SelfGroupsWordGroup& w : lay.wordGroups) {
            std::unique_ptr<Group> g(new Group);
            g->words = w.words; g->qt = w.qt; g->tiles = w.tiles; g->wordSteps = w.wordSteps;
            g->numItems = (int)(w.items.size() / 3);
            if (allocGroup(*g, w.perm)) return 1;
            EDLIB_AMD_HIP(g->d_rank.alloc(g->slots)); EDLIB_AMD_HIP(g->d_end.alloc(g->slots));
            EDLIB_AMD_HIP(g->d_items.alloc(std::max<size_t>(w.items.size(), 3)));
            EDLIB_AMD_HIP(hipMemcpy(g->d_rank.p, w.rank.data(), g->slots * sizeof(int), hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(g->d_end.p, w.end.data(), g->slots * sizeof(int), hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(g->d_items.p, w.items.data(), w.items.size() * sizeof(int), hipMemcpyHostToDevice));
            groups_.push_back(std::move(g));
        }
    }

    // ---- the pairs answered off the kernel, inside their groups: those with an empty sequence here, the rest by one pair batch
    auto members = [&](int i) { return std::make_pair(byGroup.begin() + memberOff[groupOf[i]], byGroup.begin() + memberOff[groupOf[i] + 1]); };
    for (int e : empties) {
        const auto m = members(e);
        for (auto it = m.first; it != m.second; ++it) {
            const int x = *it;
            if (x == e || (len(x) == 0 && x < e)) continue;          // two empty sequences: once
            selfOther_.push_back(key(e, x));
            selfEmptyVal_.push_back(len(x));
        }
    }
    {
        PairPool pool;
        long long np = 0;
        std::vector<char> isOut(n, 0);
        for (int i : outK) isOut[i] = 1;
        for (int i : outK) {
            const auto m = members(i);
            for (auto it = m.first; it != m.second && np <= 0x7fffffffLL; ++it) {
                const int x = *it;
                if (x == i || len(x) == 0 || (isOut[x] && x < i)) continue;   // two such sequences: once
                if (!inWindow(i, x) || ++np > 0x7fffffffLL) continue;
                const int lo = std::min(i, x), hi = std::max(i, x);
                pool.add(seqs + off[lo], len(lo), false, seqs + off[hi], len(hi));
                selfOther_.push_back(key(lo, hi));
            }
        }
        if (np > 0x7fffffffLL) {
            set_error("grouped self batch: too many pairs outside the kernel's envelope (more than 2^31 - 1): sequences above "
                      "%d bases or a set with more than %d symbols", 32 * kCrossMaxQueryWords, kCrossMaxSyms);
            return 1;
        }
        if (np > 0) {
            longPairs_.reset(new Batch);
            if (pool.init(*longPairs_, cfg_, device)) return 1;
        }
    }
    otherCells_ = (long long)selfOther_.size();
    if (otherCells_ > 0) {
        EDLIB_AMD_HIP(h_vals_.alloc((size_t)otherCells_ * sizeof(int)));
        std::copy(selfEmptyVal_.begin(), selfEmptyVal_.end(), reinterpret_cast<int*>(h_vals_.p));
    }
    return 0;
}

int CrossBatch::runSelf()
{
    pool_quarantine(false);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard guard(device_);
    if (beginRun(guard.status, {&mat_, &near_, &hitList_.result, &cellStrand_, &bestStrand_})) return 1;
    if (hits_) EDLIB_AMD_HIP(hitList_.reset(stream_));
    // the pairs outside the length window are visited by no work item and are in no pair batch: -1 from here
    else if (cfg_.k >= 0 && cells_ > 0) {
        EDLIB_AMD_HIP(hipMemsetAsync(d_mat_.p, 0xff, cells_ * sizeof(int), stream_));
        if (strands_) EDLIB_AMD_HIP(hipMemsetAsync(d_smat_.p, 0, cells_, stream_));
    }

    if (scanRun(groups_, 8, [&] { return scanGroups(); })) return 1;
    otherHits_.clear();
    if (otherCells_ > 0) {
        int* vals = reinterpret_cast<int*>(h_vals_.p);
        uint8_t* svals = strands_ ? h_svals_.p : nullptr;
        const size_t ne = selfEmptyVal_.size(), np = (size_t)otherCells_ - ne;
        if (longPairs_) {
            if (longPairs_->run()) return 1;
            const size_t per = strands_ ? 2 : 1;
            std::vector<int> rec(3 * per * np);
            if (gather(*longPairs_, per * np, rec.data(), nullptr)) return 1;
            for (size_t c = 0; c < np; ++c) {
                if (!strands_) { vals[ne + c] = rec[3 * c]; continue; }
                // the pairs 2c (forward) and 2c + 1 (reverse complement) of every pair, decided here
                const int w = resolve_strands(rec[6 * c], rec[6 * c + 3]);
                vals[ne + c] = rec[6 * c + ((w & kStrandReverse) ? 3 : 0)];
                svals[ne + c] = (uint8_t)(w & (kStrandReverse | kStrandBoth));
            }
            addSessionStats(*longPairs_, false);
        }
        if (!hits_) {
            EDLIB_AMD_HIP(hipMemcpyAsync(d_vals_.p, vals, (size_t)otherCells_ * sizeof(int), hipMemcpyHostToDevice, stream_));
            EDLIB_AMD_HIP(launch_self_scatter(d_cells_.p, d_vals_.p, otherCells_, d_mat_.p, stream_));
            if (strands_) {
                EDLIB_AMD_HIP(hipMemcpyAsync(d_svals_.p, svals, (size_t)otherCells_, hipMemcpyHostToDevice, stream_));
                EDLIB_AMD_HIP(launch_cross_scatter_bytes(d_cells_.p, d_svals_.p, otherCells_, d_smat_.p, stream_));
            }
        } else {
            // their pairs within k: ed, nloc, end (NW: one location, the last column; only the distance is reported)
            for (long long c = 0; c < otherCells_; ++c) {
                if (vals[c] == -1) continue;
                otherHits_.key.push_back(selfOther_[(size_t)c]);
                otherHits_.val[0].push_back(vals[c]); otherHits_.val[1].push_back(1); otherHits_.val[2].push_back(-1);
                if (strands_) otherHits_.byte.push_back(svals[c]);
            }
        }
    }
    if (hits_) {
        if (finishHits()) return 1;
        EDLIB_AMD_HIP(launch_self_nearest_hits(d_best_.p, nq_, d_near_.p, stream_));
        if (strands_)
            EDLIB_AMD_HIP(launch_self_nearest_strand_hits(d_best_.p, d_sbest_.p, nq_, d_sbest_.p + 2 * (size_t)nq_, stream_));
    } else {
        EDLIB_AMD_HIP(launch_self_nearest_dense(d_mat_.p, nq_, d_near_.p, stream_));
        if (strands_)
            EDLIB_AMD_HIP(launch_self_nearest_strand_dense(d_smat_.p, d_near_.p, nq_, d_sbest_.p + 2 * (size_t)nq_, stream_));
    }
    return endRun(t0, !groups_.empty());
}

int CrossBatch::selfView(int what, EdlibAmdSelfView* out)
{
    if (!haveRun_) { set_error("self batch: no results (Run it first)"); return 1; }
    if (what & ~(EDLIB_AMD_SELF_DISTANCES | EDLIB_AMD_SELF_NEAREST)) { set_error("self view: unknown parts %d", what); return 1; }
    if (hits_) what &= ~EDLIB_AMD_SELF_DISTANCES;               // a hit-list batch keeps no condensed vector
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t matBytes = cells_ * sizeof(int), nearBytes = 3 * (size_t)nq_ * sizeof(int);
    if (fetchParts({{what & EDLIB_AMD_SELF_DISTANCES, &mat_, d_mat_.p, matBytes},
                    {what & EDLIB_AMD_SELF_NEAREST, &near_, d_near_.p, nearBytes}})) return 1;
    memset(out, 0, sizeof *out);
    out->numSequences = nq_; out->numPairs = (long long)cells_;
    if (what & EDLIB_AMD_SELF_DISTANCES) out->editDistance = reinterpret_cast<const int*>(mat_.h.p);
    if (what & EDLIB_AMD_SELF_NEAREST) {
        const int* b = reinterpret_cast<const int*>(near_.h.p);
        out->nearest = b; out->nearestDistance = b + nq_; out->secondDistance = b + 2 * (size_t)nq_;
    }
    return 0;
}

int CrossBatch::selfHitsView(EdlibAmdSelfHits* out)
{
    if (!hits_) {
        set_error("edlibAmdBatchSelfHits: not a hit-list batch (create it with edlibAmdBatchCreateSelfHits; a dense self "
                  "batch has edlibAmdBatchSelfView)");
        return 1;
    }
    if (!haveRun_) { set_error("self batch: no results (Run it first)"); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    // the finished list is [4][numHits] (partner, editDistance, numLocations, endLocation): the first two planes travel
    const int* l = nullptr;
    memset(out, 0, sizeof *out);
    if (hitList_.fetch(2, stream_, &out->rowOffsets, &l)) return 1;
    out->numSequences = nq_; out->numHits = hitList_.outN;
    out->partner = l; out->editDistance = l + (size_t)hitList_.outN;
    return 0;
}

int CrossBatch::selfStrandsView(int what, EdlibAmdSelfStrands* out)
{
    if (!strands_) {
        set_error("edlibAmdBatchSelfStrands: not a both-strand self batch (create it with edlibAmdBatchCreateSelfBothStrands "
                  "or edlibAmdBatchCreateSelfHitsBothStrands)");
        return 1;
    }
    if (!haveRun_) { set_error("self batch: no results (Run it first)"); return 1; }
    if (what & ~(EDLIB_AMD_SELF_DISTANCES | EDLIB_AMD_SELF_NEAREST)) { set_error("self strands: unknown parts %d", what); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t pairBytes = hits_ ? (size_t)hitList_.outN : cells_;
    if (fetchParts({{what & EDLIB_AMD_SELF_DISTANCES, &cellStrand_, hits_ ? hitList_.byteOut.p : d_smat_.p, pairBytes},
                    {what & EDLIB_AMD_SELF_NEAREST, &bestStrand_, d_sbest_.p + 2 * (size_t)nq_, (size_t)nq_}})) return 1;
    memset(out, 0, sizeof *out);
    out->numSequences = nq_; out->numPairs = (long long)cells_; out->numHits = hits_ ? hitList_.outN : 0;
    if (what & EDLIB_AMD_SELF_DISTANCES) (hits_ ? out->hitStrand : out->pairStrand) = cellStrand_.h.p;
    if (what & EDLIB_AMD_SELF_NEAREST) out->nearestStrand = bestStrand_.h.p;
    return 0;
}

int CrossBatch::selfComponents(int maxDistance, int what, EdlibAmdSelfComponents* out)
{
    if (!haveRun_) { set_error("self batch: no results (Run it first)"); return 1; }
    if (!what || (what & ~(EDLIB_AMD_COMPONENT_LABELS | EDLIB_AMD_COMPONENT_MEMBERS))) {
        set_error("self components: unknown parts %d", what);
        return 1;
    }
    if (cfg_.k >= 0 && maxDistance > cfg_.k) {
        set_error("self components: maxDistance %d is above the batch's k = %d: the batch kept no pairs beyond k (create it "
                  "with a larger k)", maxDistance, cfg_.k);
        return 1;
    }
    const int level = maxDistance >= 0 ? maxDistance : cfg_.k;       // (k < 0 too: every reported pair)
    const bool members = (what & EDLIB_AMD_COMPONENT_MEMBERS) != 0;
    const int n = nq_;
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    EDLIB_AMD_HIP(d_comp_.ensure(SelfComponentsBuffers::ints(n)));
    const SelfComponentsBuffers b = SelfComponentsBuffers::carve(d_comp_.p, n);
    size_t scratch = 0;
    if (members && n > 0) {
        EDLIB_AMD_HIP(self_components_scratch(n, &scratch));
        EDLIB_AMD_HIP(hitList_.needScratch(scratch));
    }
    // the edges where the Run left them: the finished list's partner and distance planes with the sorted keys its finish
    // leaves behind (their high half is the row), or the condensed vector
    const long long numHits = hits_ ? hitList_.outN : 0;
    EDLIB_AMD_HIP(launch_self_components(b, n, hits_ ? hitList_.skey.p : nullptr, hits_ ? hitList_.out() : nullptr,
                                         hits_ ? hitList_.out() + (size_t)numHits : nullptr, numHits,
                                         hits_ ? nullptr : d_mat_.p, level, members, hitList_.tmp.p, hitList_.tmp.n, stream_));
    // label, componentSize, numComponents and -- behind them on the device -- the offsets and members: one copy
    const size_t ints = n > 0 ? (members ? 4 * (size_t)n + 3 : 2 * (size_t)n + 1) : 0;
    comp_.fetched = false;
    EDLIB_AMD_HIP(comp_.fetch(d_comp_.p, ints * sizeof(int), stream_, 0, 4 * sizeof(int)));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    comp_.fetched = true;
    if (n == 0) memset(comp_.h.p, 0, 4 * sizeof(int));             // no component: componentOffsets is {0}
    const int* h = reinterpret_cast<const int*>(comp_.h.p);
    memset(out, 0, sizeof *out);
    out->numSequences = n;
    out->numComponents = n > 0 ? h[2 * (size_t)n] : 0;
    out->label = h; out->componentSize = h + n;
    if (members) { out->componentOffsets = h + (b.offsets - b.label); out->members = h + (b.members - b.label); }
    return 0;
}

int CrossBatch::selfNeighbors(int K, int maxDistance, EdlibAmdNeighbors* out)
{
    int level = -1;
    if (!haveRun_) { set_error("self batch: no results (Run it first)"); return 1; }
    if (neighborsLevel("self neighbors", K, maxDistance, &level)) return 1;
    const int n = nq_;
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    NeighborsSource src{};
    src.numRows = n; src.rowLength = n;
    if (!hits_) {
        // the condensed vector as it lies there: row i is its stretch of row i and one cell of every row above
        src.kind = NeighborsSource::kCondensed;
        src.ed = d_mat_.p;
        src.strand = strands_ ? d_smat_.p : nullptr;
    } else {
        // the finished list holds a pair once, under its lower index: mirrored into a CSR with every pair under both ends
        const long long numHits = hitList_.outN;
        size_t scratch = 0;
        if (n > 0) {
            EDLIB_AMD_HIP(neighbors_mirror_scratch(n, &scratch));
            EDLIB_AMD_HIP(hitList_.needScratch(scratch));
        }
        EDLIB_AMD_HIP(d_mirror_.ensure(NeighborsMirror::bytes(n, numHits)));
        const NeighborsMirror m = NeighborsMirror::carve(d_mirror_.p, n, numHits);
        EDLIB_AMD_HIP(launch_neighbors_mirror(m, n, hitList_.skey.p, hitList_.out(), hitList_.out() + (size_t)numHits, numHits,
                                              hitList_.tmp.p, hitList_.tmp.n, stream_));
        src.kind = NeighborsSource::kCsr;
        src.off = m.off; src.partner = m.partner; src.distance = m.distance; src.position = m.position;
        src.strand = strands_ ? hitList_.byteOut.p : nullptr;
    }
    return selectNeighbors(src, K, level, out);
}

}  // namespace edlib_amd
