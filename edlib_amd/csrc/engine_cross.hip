// engine_cross.hip -- host side of cross batches: every query against every target, DISTANCE only (DESIGN.md "Cross
// batches").  Create sorts the queries into word groups (kernel A's groups, each sorted by length) and the targets by
// length, packs the targets to 4-bit codes once and chooses each group's tile; a Run builds the Peq rows of every query
// (build_peq_reads_kernel over the union target alphabet), scans every group on the cross kernel, lets the internal
// sessions of the cells outside the kernel's envelope run meanwhile, scatters their results into the matrix and reduces
// it to the best hits.  Results stay in HBM until view() asks for a part of them.  A hit-list batch appends the cells
// within k instead (the scan, then the internal sessions' cells behind them) and finishes the list on the device
// (hit_list.hpp, cross_hits.hip): sorted into CSR order, target offsets, best hits from the list.
// A both-strand batch makes the pool of every query and its reverse complement on the device, gives mates
// the slots s and s ^ 1 of their word group, and keeps a strand byte beside every cell, hit and best hit.
// An occurrence batch (DESIGN.md §4h "Occurrence batches") is a hit-list batch whose entries are the maximal runs of
// columns within k of every cell: the occurrence scan appends them, each target outside the kernel's envelope runs through
// an internal hit-list shared-target session, and the finish sorts the runs into CSR order without best hits.
// setTargets (DESIGN.md §4h "Streamed targets") passes another target set through the resident batch: the set is prepared
// on the device (cross_targets.hip: census, order by length, packed offsets; the way init prepares a set within the
// kernel's target length), swapped in once it is known to lie inside the kernel's envelope, and the groups are shaped
// again (shapeGroups, init's own).
#include "engine_lanes.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace edlib_amd {

// lanes a tile shape leaves idle decide it; on a tie the wider query tile (fewer Peq stagings)
// (minQt = 2 for both strands: nq counts slots, mates are neighbouring lanes)
int choose_qt(long long nq, long long nt, int minQt)
{
    int bestQt = 64; long long bestLanes = -1;
    for (int qt = 64; qt >= minQt; qt >>= 1) {
        const long long tpt = 64 / qt;
        const long long lanes = ((nq + qt - 1) / qt) * qt * ((nt + tpt - 1) / tpt) * tpt;
        if (bestLanes < 0 || lanes < bestLanes) { bestLanes = lanes; bestQt = qt; }
    }
    return bestQt;
}

// the host's share of a set, linear in its count: colsBelow[L] = columns of the targets shorter than L (L up to the
// longest + 1), the dwords of the packed pool
static void columns_by_length(const long long* toff, int nt, int maxLen, std::vector<long long>& colsBelow, long long* dwords)
{
    colsBelow.assign((size_t)maxLen + 2, 0);
    *dwords = 0;
    for (int t = 0; t < nt; ++t) {
        const long long n = toff[t + 1] - toff[t];
        colsBelow[(size_t)n + 1] += n;
        *dwords += (n + 7) / 8;
    }
    for (size_t l = 1; l < colsBelow.size(); ++l) colsBelow[l] += colsBelow[l - 1];
}

int CrossBatch::init(const char* queries, const long long* qoffIn, int nq, const char* targets,
                     const long long* toffIn, int nt, EdlibAlignConfig cfg, int device, bool hits, bool strands, bool occ)
{
    std::vector<long long> qoff, toff;
    if (occ) {
        // what an occurrence batch takes (edlib_amd.h): everything else is refused with the limit named, before the device
        if (cfg.mode != EDLIB_MODE_HW) {
            set_error("occurrence cross batch: config.mode must be EDLIB_MODE_HW (NW and SHW have no occurrence list)");
            return 1;
        }
        if (cfg.task != EDLIB_TASK_DISTANCE) {
            set_error("occurrence cross batch: config.task must be EDLIB_TASK_DISTANCE (start locations and paths: align "
                      "the chosen windows with a pair or window batch)");
            return 1;
        }
        if (cfg.k < 0) { set_error("occurrence cross batch: config.k must be >= 0 (got %d)", cfg.k); return 1; }
        if (nq < 0 || nt < 0 || (nq > 0 && !qoffIn) || (nt > 0 && !toffIn) || strands || !hits) { set_error("bad batch shape"); return 1; }
        if (copy_offsets(qoffIn, nq, "query", qoff) || copy_offsets(toffIn, nt, "target", toff)) return 1;
        for (int q = 0; q < nq; ++q)
            if (qoff[q + 1] - qoff[q] > 32LL * kCrossMaxQueryWords) {
                set_error("occurrence cross batch: query %d has %lld bases, the limit is %d", q, qoff[q + 1] - qoff[q],
                          32 * kCrossMaxQueryWords);
                return 1;
            }
        for (int t = 0; t < nt; ++t) {
            unsigned long long seen[4] = {0, 0, 0, 0};
            for (long long j = toff[t]; j < toff[t + 1]; ++j) { const uint8_t c = (uint8_t)targets[j]; seen[c >> 6] |= 1ull << (c & 63); }
            const int sigma = __builtin_popcountll(seen[0]) + __builtin_popcountll(seen[1]) + __builtin_popcountll(seen[2]) +
                              __builtin_popcountll(seen[3]);
            if (sigma > kCrossMaxSyms) {
                set_error("occurrence cross batch: target %d has %d distinct symbols, the limit is %d", t, sigma, kCrossMaxSyms);
                return 1;
            }
        }
    }
    if (cfg.task != EDLIB_TASK_DISTANCE) {
        set_error("cross batches compute distances only (EDLIB_TASK_DISTANCE): align the chosen pairs with a pair batch "
                  "for locations or paths");
        return 1;
    }
    if (hits && cfg.k < 0) {
        set_error("hit-list cross batches need config.k >= 0 (every cell is a hit at k = %d: use edlibAmdBatchCreateCross "
                  "for the dense matrix)", cfg.k);
        return 1;
    }
    if (cfg.mode != EDLIB_MODE_NW && cfg.mode != EDLIB_MODE_SHW && cfg.mode != EDLIB_MODE_HW) { set_error("unknown mode"); return 1; }
    if (nq < 0 || nt < 0 || (nq > 0 && !qoffIn) || (nt > 0 && !toffIn)) { set_error("bad batch shape"); return 1; }
    if (strands && nq > 0x3fffffff) { set_error("bad both-strand batch shape"); return 1; }
    if (check_device(device)) return 1;
    keep_config(cfg, cfg_, eqs_);
    device_ = device; nq_ = nq; nt_ = nt; hits_ = hits; strands_ = strands; occ_ = occ;
    if (!occ && (copy_offsets(qoffIn, nq, "query", qoff) || copy_offsets(toffIn, nt, "target", toff))) return 1;
    const long long tb = toff[0];
    const long long qbytes = qoff[nq] - qoff[0], tbytes = toff[nt] - tb;
    auto qlen = [&](int q) { return (int)(qoff[q + 1] - qoff[q]); };
    auto tlen = [&](int t) { return (int)(toff[t + 1] - toff[t]); };
    cells_ = (size_t)nq * (size_t)nt;
    stats = EdlibAmdBatchStats{};
    stats.cells = qbytes * tbytes * (strands ? 2 : 1);

    // the queries as every target set finds them: word groups, each sorted by length; empty queries ride in the
    // one-word group
    std::vector<int> longQ;
    qbytes_ = qbytes;
    qlen_.resize((size_t)nq);
    wordQueries_.assign(kCrossMaxQueryWords + 1, std::vector<int>());
    for (int q = 0; q < nq; ++q) {
        const int m = qlen_[q] = qlen(q);
        if (m > maxQlen_) { maxQlen_ = m; longestQuery_ = q; }
        if (m > 32 * kCrossMaxQueryWords) longQ.push_back(q);
        else wordQueries_[std::max(1, (m + 31) / 32)].push_back(q);
    }
    for (auto& qs : wordQueries_)
        std::stable_sort(qs.begin(), qs.end(), [&](int a, int b) { return qlen_[a] < qlen_[b]; });

    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    if (openStream()) return 1;
    if (sizeResults()) return 1;

    // the union alphabet of all targets decides the Peq rows (and whether the kernel can take any cell).  A set whose
    // every target fits the kernel's length is prepared on the device, the way setTargets does it; one with a longer
    // target is read on the host, and the targets the kernel takes are packed from there.
    int maxTlen = 0;
    for (int t = 0; t < nt; ++t) maxTlen = std::max(maxTlen, tlen(t));
    const bool deviceSet = nt > 0 && maxTlen <= kCrossMaxTarget;
    TargetPrep prep;
    std::vector<long long> colsBelow;
    if (deviceSet) {
        long long dwords = 0;
        columns_by_length(toff.data(), nt, maxTlen, colsBelow, &dwords);
        if (prepareTargets(targets, toff.data(), nt, dwords, prep, tab_)) return 1;
    } else build_tables(tab_, reinterpret_cast<const uint8_t*>(targets) + tb, tbytes, eqs_.data(), (int)eqs_.size());
    const bool wide = tab_.sigmaT > kCrossMaxSyms;
    syms_ = peq_syms(tab_.sigmaT);
    std::vector<int> inT;
    for (int t = 0; t < nt; ++t) {
        if (!wide && tlen(t) <= kCrossMaxTarget) inT.push_back(t);
        else outTargets_.push_back(t);
    }

    // ---- the cross kernel's share
    const bool kernelShare = !inT.empty() && (int)longQ.size() < nq;
    // (what a pair batch that gathers from this one is checked against: gatherSource)
    tlenHost_.resize((size_t)nt);
    for (int t = 0; t < nt; ++t) tlenHost_[t] = tlen(t);
    inPack_.assign((size_t)nt, 0);
    if (kernelShare)
        for (int t : inT) inPack_[t] = 1;
    // (queries the kernel can take are resident even where this set leaves it nothing: a later setTargets finds them)
    if ((kernelShare || (nq > 0 && longQ.empty())) && uploadQueries(queries, qoff, strands_)) return 1;
    if (kernelShare && deviceSet) {
        if (adoptTargets(prep, nt)) return 1;
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        numSorted_ = nt; sortedCols_ = tbytes;
        if (shapeGroups(colsBelow)) return 1;
    } else if (kernelShare) {
        std::stable_sort(inT.begin(), inT.end(), [&](int a, int b) { return tlen(a) < tlen(b); });
        numSorted_ = (int)inT.size();
        std::vector<int> tl(numSorted_);
        for (int i = 0; i < numSorted_; ++i) {
            tl[i] = tlen(inT[i]);
            sortedCols_ += tl[i];
        }
        colsBelow.assign((size_t)tl.back() + 2, 0);
        for (int l : tl) colsBelow[(size_t)l + 1] += l;
        for (size_t l = 1; l < colsBelow.size(); ++l) colsBelow[l] += colsBelow[l - 1];
        if (packHostTargets(targets, toff, inT, tl)) return 1;
        EDLIB_AMD_HIP(d_tlen_.alloc(numSorted_));
        EDLIB_AMD_HIP(hipMemcpy(d_tlen_.p, tl.data(), numSorted_ * sizeof(int), hipMemcpyHostToDevice));
        if (shapeGroups(colsBelow)) return 1;
    }

    // ---- the other engines' share
    if (nq > 0) {
        for (int t : outTargets_) {
            std::unique_ptr<Batch> b(new Batch);
            const long long to[2] = {toff[t], toff[t + 1]};
            if (b->init(queries, qoffIn, nq, targets, to, 1, cfg_, device, strands_, /*hits=*/occ_)) return 1;
            outShared_.push_back(std::move(b));
            if (!occ_) otherCells_ += nq;             // (an occurrence batch reads the sessions' own lists)
        }
        if (!longQ.empty() && !inT.empty()) {
            // every long query against every target the kernel takes, as pairs (their bytes replicated per cell)
            PairPool pool;
            // (both strands: the pairs 2c and 2c + 1 of cell c, the second with the reverse complement made here)
            for (int t : inT)
                for (int q : longQ) {
                    for (int st = 0; st < (strands_ ? 2 : 1); ++st)
                        pool.add(queries + qoff[q], qlen(q), st != 0, targets + toff[t], tlen(t));
                    longCells_.push_back((long long)t * nq + q);
                }
            if (pool.size() > 0x7fffffffLL) {
                set_error("cross batch: too many cells of long queries (%lld pairs)", pool.size());
                return 1;
            }
            longPairs_.reset(new Batch);
            if (pool.init(*longPairs_, cfg_, device)) return 1;
            otherCells_ += (long long)longCells_.size();
        }
        if (otherCells_ > 0) {
            std::vector<long long> cellIdx;
            cellIdx.reserve((size_t)otherCells_);
            for (int t : outTargets_)
                for (int q = 0; q < nq; ++q) cellIdx.push_back((long long)t * nq + q);
            cellIdx.insert(cellIdx.end(), longCells_.begin(), longCells_.end());
            EDLIB_AMD_HIP(h_vals_.alloc(3 * (size_t)otherCells_ * sizeof(int)));
            if (strands_) {
                EDLIB_AMD_HIP(h_svals_.alloc((size_t)otherCells_));
                if (!hits_) EDLIB_AMD_HIP(d_svals_.alloc((size_t)otherCells_));
            }
            if (hits_) otherCellIdx_.swap(cellIdx);            // their hits are appended from the host
            else {
                EDLIB_AMD_HIP(d_cells_.alloc((size_t)otherCells_)); EDLIB_AMD_HIP(d_vals_.alloc(3 * (size_t)otherCells_));
                EDLIB_AMD_HIP(hipMemcpy(d_cells_.p, cellIdx.data(), (size_t)otherCells_ * sizeof(long long), hipMemcpyHostToDevice));
            }
        }
    }
    return 0;
}

// the result buffers of nq_ x nt_ cells: made where there are none, grown where the counts need more, otherwise kept (a
// hit list keeps the capacity an earlier Run grew it to)
int CrossBatch::sizeResults()
{
    const size_t nq = (size_t)nq_, nt = (size_t)nt_;
    if (!occ_) EDLIB_AMD_HIP(d_best_.ensure(3 * nt + 3 * nq));
    if (strands_) {
        EDLIB_AMD_HIP(d_sbest_.ensure(std::max<size_t>(nt + nq, 1)));
        if (!hits_) EDLIB_AMD_HIP(d_smat_.ensure(std::max<size_t>(cells_, 1)));
    }
    if (!hits_) {
        EDLIB_AMD_HIP(d_mat_.ensure(3 * std::max<size_t>(cells_, 1)));
        targetChunk_ = std::max(1024, (nt_ + 32767) / 32768);
        EDLIB_AMD_HIP(d_partial_.ensure((size_t)std::max(1, (nt_ + targetChunk_ - 1) / targetChunk_) * std::max<size_t>(nq, 1)));
    } else {
        if (!occ_) EDLIB_AMD_HIP(d_bkey_.ensure(2 * (nt + nq)));
        if (sizeHitList(std::max<long long>(1LL << 20, (long long)nq_ + nt_))) return 1;
    }
    return 0;
}

int CrossBatch::sizeHitList(long long minCap)
{
    // (2^32 - 1 entries: the sort's index)
    hitList_.configure("cross batch", occ_ ? "runs" : "hits", occ_ ? 5 : 3, 32, strands_, 0);
    return hitList_.size((size_t)nt_, minCap, stream_);
}

int CrossBatch::shapeGroups(const std::vector<long long>& colsBelow)
{
    std::vector<std::unique_ptr<Group>> kept;
    kept.swap(groups_);
    if (numSorted_ == 0) return 0;
    const long long top = (long long)colsBelow.size() - 1;
    // columns the kernel scans for a query of length m: all of them, or under NW with k >= 0 those of the targets in
    // the length window [m - k, m + k] (cross_nw_outside)
    auto scannedCols = [&](int m) -> long long {
        if (cfg_.mode == EDLIB_MODE_NW && cfg_.k >= 0) {
            const long long lo = std::min(std::max((long long)m - cfg_.k, 0LL), top);
            const long long hi = std::min((long long)m + cfg_.k + 1, top);
            return colsBelow[(size_t)hi] - colsBelow[(size_t)lo];
        }
        return sortedCols_;
    };
    for (int w = 1; w <= kCrossMaxQueryWords; ++w) {
        const auto& qs = wordQueries_[w];
        if (qs.empty()) continue;
        std::unique_ptr<Group> g;
        for (auto& o : kept)
            if (o && o->words == w) g = std::move(o);
        if (!g) { g.reset(new Group); g->words = w; }
        // both strands: each query of the sorted list becomes two slots, itself and its reverse complement
        const long long need = (long long)qs.size() * (strands_ ? 2 : 1);
        const int qt = choose_qt(need, numSorted_, strands_ ? 2 : 1);
        const bool fresh = g->slots == 0 || qt != g->qt || g->syms != syms_;
        g->qt = qt;
        g->tiles = (int)((need + g->qt - 1) / g->qt);
        g->wordSteps = 0;
        for (int q : qs) g->wordSteps += (long long)w * scannedCols(qlen_[q]) * (strands_ ? 2 : 1);
        const int tpt = 64 / g->qt;
        const long long targetTiles = (numSorted_ + tpt - 1) / tpt;
        // about 8,192 waves per launch (256 CUs), each persistent over a strided range of target tiles
        g->ysplit = (int)std::min<long long>({targetTiles, std::max(1LL, (8192LL + g->tiles - 1) / g->tiles), 65535LL});
        if (fresh) {
            std::vector<int> perm((size_t)g->tiles * g->qt, -1);           // whole tiles
            if (!strands_) std::copy(qs.begin(), qs.end(), perm.begin());
            else {
                for (size_t i = 0; i < qs.size(); ++i) { perm[2 * i] = 2 * qs[i]; perm[2 * i + 1] = 2 * qs[i] + 1; }
                // what the kernel's lane exchange rests on: mates in the slots s and s ^ 1, padding in pairs, an even tile
                bool ok = !(g->qt & 1) && !(perm.size() & 1);
                for (size_t sl = 0; ok && sl < perm.size(); sl += 2)
                    ok = perm[sl] < 0 ? perm[sl + 1] < 0 : (!(perm[sl] & 1) && perm[sl + 1] == perm[sl] + 1);
                if (!ok) { set_error("both strands: mates are not in adjacent slots"); return 1; }
            }
            if (allocGroup(*g, perm)) return 1;
            g->syms = syms_;
        }
        groups_.push_back(std::move(g));
    }
    return 0;
}

// A target set (every target at most kCrossMaxTarget bases) on its way into the batch: the raw pool and the caller's
// offsets go up as they are, one asynchronous copy each, and the device makes the rest (cross_targets.hip) -- the presence
// set of the pool, the stable order by length, the dword offsets of the packed targets.  `dwords`: of the packed pool.
// tab: the tables of the bytes the census found with the batch's equalities, symbol ids in ascending byte order (nothing
// a cross batch reports depends on the ids: tlut and eqtbl only have to agree).  The stream is idle afterwards; nothing
// of the batch has changed.
int CrossBatch::prepareTargets(const char* targets, const long long* toffIn, int nt, long long dwords, TargetPrep& p,
                               Tables& tab)
{
    if (!h_census_.p) EDLIB_AMD_HIP(h_census_.alloc(8 * sizeof(uint32_t)));
    uint32_t* presence = reinterpret_cast<uint32_t*>(h_census_.p);
    memset(presence, 0, 8 * sizeof(uint32_t));
    if (nt > 0) {
        const size_t n = (size_t)nt;
        const long long tbytes = toffIn[nt] - toffIn[0];
        size_t tmpBytes = 0;
        EDLIB_AMD_HIP(cross_targets_order_bytes(nt, &tmpBytes));
        EDLIB_AMD_HIP(p.raw.alloc((size_t)tbytes + 16)); EDLIB_AMD_HIP(p.offIn.alloc(n + 1)); EDLIB_AMD_HIP(p.offR.alloc(n + 1));
        EDLIB_AMD_HIP(p.pres.alloc(8)); EDLIB_AMD_HIP(p.len.alloc(n)); EDLIB_AMD_HIP(p.idx.alloc(n));
        EDLIB_AMD_HIP(p.dw.alloc(n)); EDLIB_AMD_HIP(p.tmp.alloc(tmpBytes)); EDLIB_AMD_HIP(p.tlut.alloc(256));
        EDLIB_AMD_HIP(p.tlen.alloc(n)); EDLIB_AMD_HIP(p.tperm.alloc(n)); EDLIB_AMD_HIP(p.tdw.alloc(n));
        EDLIB_AMD_HIP(p.tpk.alloc((size_t)std::max(dwords, 1LL)));
        if (tbytes) EDLIB_AMD_HIP(hipMemcpyAsync(p.raw.p, targets + toffIn[0], (size_t)tbytes, hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(p.offIn.p, toffIn, (n + 1) * sizeof(long long), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(launch_cross_targets_prepare(p.raw.p, p.offIn.p, nt, p.offR.p, p.pres.p, p.len.p, p.idx.p, p.tlen.p,
                                                   p.tperm.p, p.dw.p, p.tdw.p, p.tmp.p, tmpBytes, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(presence, p.pres.p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    }
    uint8_t present[256];
    int numPresent = 0;
    for (int b = 0; b < 256; ++b)
        if (presence[b >> 5] >> (b & 31) & 1) present[numPresent++] = (uint8_t)b;
    build_tables(tab, present, numPresent, eqs_.data(), (int)eqs_.size());
    return 0;
}

// the prepared set packed with tab_'s codes and made the batch's (what the batch held goes into p and dies with it: the
// caller synchronises the stream before that)
int CrossBatch::adoptTargets(TargetPrep& p, int nt)
{
    if (nt == 0) return 0;
    EDLIB_AMD_HIP(hipMemcpyAsync(p.tlut.p, tab_.tlut, 256, hipMemcpyHostToDevice, stream_));
    EDLIB_AMD_HIP(launch_pack_cross_targets(p.raw.p, p.offR.p, p.tperm.p, p.tdw.p, nt, p.tlut.p, p.tpk.p, stream_));
    d_tpk_.swap(p.tpk); d_tdw_.swap(p.tdw); d_tperm_.swap(p.tperm); d_tlen_.swap(p.tlen);
    return 0;
}

int CrossBatch::setTargets(const char* targets, const long long* toffIn, int nt)
{
    static const char* const fn = "edlibAmdBatchCrossSetTargets";
    // ---- what is refused leaves the batch as it was
    if (self_) { set_error("%s: not available on a self batch", fn); return 1; }
    if (nt < 0) { set_error("%s: numTargets must be >= 0 (got %d)", fn, nt); return 1; }
    if (nt > 0 && (!targets || !toffIn)) { set_error("%s: targets and targetOffsets must not be NULL for %d targets", fn, nt); return 1; }
    if (maxQlen_ > 32 * kCrossMaxQueryWords) {
        set_error("%s: query %d has %s bases, the limit for a batch that streams targets is %d: create a new batch", fn,
                  longestQuery_, with_commas(maxQlen_).c_str(), 32 * kCrossMaxQueryWords);
        return 1;
    }
    // the host's share, linear in numTargets: the offsets checked, the longest target, the columns by length
    int maxLen = 0;
    std::vector<int> tlens((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        const long long n = toffIn[t + 1] - toffIn[t];
        if (n < 0) { set_error("%s: bad target offsets (target %d ends before it starts)", fn, t); return 1; }
        if (n > kCrossMaxTarget) {
            set_error("%s: target %d has %s bases, the limit for a streamed set is %s: create a new batch", fn, t,
                      with_commas(n).c_str(), with_commas(kCrossMaxTarget).c_str());
            return 1;
        }
        maxLen = std::max(maxLen, (int)n);
        tlens[(size_t)t] = (int)n;
    }
    const long long tbytes = nt > 0 ? toffIn[nt] - toffIn[0] : 0;
    std::vector<long long> colsBelow;
    long long dwords = 0;
    columns_by_length(toffIn, nt, maxLen, colsBelow, &dwords);

    // ---- the set prepared into buffers of its own: the pool and the offsets go up as they are, the device does the rest
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    TargetPrep prep;
    Tables tab;
    if (prepareTargets(targets, toffIn, nt, dwords, prep, tab)) return 1;
    if (tab.sigmaT > kCrossMaxSyms) {
        set_error("%s: the targets hold %d distinct symbols, the limit for a streamed set is %d: create a new batch", fn,
                  tab.sigmaT, kCrossMaxSyms);
        return 1;
    }

    // ---- swapped in; from here a device error leaves the batch without targets
    noTargets_ = true;
    haveRun_ = false;
    tab_ = tab;
    syms_ = peq_syms(tab_.sigmaT);
    EDLIB_AMD_HIP(d_eqtbl_.ensure(256)); EDLIB_AMD_HIP(d_presence_.ensure(8));
    EDLIB_AMD_HIP(hipMemcpyAsync(d_eqtbl_.p, tab_.eqtbl, 512, hipMemcpyHostToDevice, stream_));
    EDLIB_AMD_HIP(hipMemcpyAsync(d_presence_.p, tab_.presence, 32, hipMemcpyHostToDevice, stream_));
    if (adoptTargets(prep, nt)) return 1;
    // (every target of a streamed set is in the pack; the places of the set before go with it: gatherSource)
    tlenHost_.swap(tlens);
    inPack_.assign((size_t)nt, 1);
    placeReady_ = false;
    // the internal sessions of the set before are gone with it: a streamed set needs none
    outShared_.clear(); outTargets_.clear(); longPairs_.reset(); longCells_.clear(); otherCellIdx_.clear();
    otherCells_ = 0;
    nt_ = nt; numSorted_ = nt; sortedCols_ = tbytes;
    cells_ = (size_t)nq_ * (size_t)nt;
    hitList_.n = hitList_.outN = 0;
    stats = EdlibAmdBatchStats{};
    stats.cells = qbytes_ * tbytes * (strands_ ? 2 : 1);
    if (sizeResults() || shapeGroups(colsBelow)) return 1;
    // (the raw pool and the scratch die here, the set before dies here: behind the pack)
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    noTargets_ = false;
    return 0;
}

int CrossBatch::gatherSource(const char* fn, CellSource& out)
{
    const char* const what = self_ ? "the self batch" : occ_ ? "the occurrence batch" : "the cross batch";
    if (noTargets_) {
        set_error("%s: %s has no targets (edlibAmdBatchCrossSetTargets failed on the device): set them again", fn, what);
        return 1;
    }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const bool packed = numSorted_ > 0 && d_tpk_.p && d_tdw_.p && d_tperm_.p && d_qpool_.p && d_qoff_.p;
    if (packed && !placeReady_) {
        EDLIB_AMD_HIP(d_place_.ensure((size_t)nt_));
        EDLIB_AMD_HIP(launch_pack_places(d_tperm_.p, numSorted_, d_place_.p, nt_, stream_));
    }
    // (Create and SetTargets end with work of theirs in flight; the gather runs on the pair batch's stream)
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    if (packed) placeReady_ = true;
    out = CellSource{};
    out.what = what; out.self = self_;
    out.numQueries = nq_; out.numTargets = nt_;
    out.h_qlen = self_ ? tlenHost_.data() : qlen_.data();
    out.h_tlen = tlenHost_.data();
    out.h_inPack = packed ? inPack_.data() : nullptr;
    out.d_qpool = d_qpool_.p; out.qpoolBytes = d_qpool_.n; out.d_qoff = d_qoff_.p; out.stranded = strands_;
    out.d_pack = d_tpk_.p; out.packDwords = (long long)d_tpk_.n; out.d_tdw = d_tdw_.p; out.d_place = d_place_.p;
    memcpy(out.idToByte, tab_.idToByte, 16);
    return 0;
}

int CrossBatch::noResults()
{
    if (noTargets_)
        set_error("cross batch: it has no targets (edlibAmdBatchCrossSetTargets failed on the device): set them again");
    else set_error("cross batch: no results (Run it first)");
    return 1;
}

// editDistance / numLocations / first end location of the n units of an internal session's last run; sbytes (a both-strand
// session): their strand bytes
int CrossBatch::gather(Batch& b, size_t n, int* vals, uint8_t* sbytes)
{
    if (readCells(b, n, vals, "cross")) return 1;
    if (sbytes) {
        EdlibAmdStrandView sv{};
        if (b.strandView(&sv)) return 1;
        for (size_t i = 0; i < n; ++i)
            sbytes[i] = vals[3 * i] < 0 ? 0 : (uint8_t)((sv.strand[i] ? kStrandReverse : 0) | (sv.bothStrands[i] ? kStrandBoth : 0));
    }
    return 0;
}

// one scan per word group (the Peq is built; a hit-list batch's counter is reset)
int CrossBatch::scanGroups()
{
    for (auto& g : groups_) {
        CrossScanArgs a{};
        a.peq = g->d_peq.p; a.qlen = g->d_qlen.p; a.qperm = g->d_perm.p; a.qt = g->qt; a.numQueryTiles = g->tiles;
        a.tpk = d_tpk_.p; a.tdw = d_tdw_.p; a.tlen = d_tlen_.p; a.tperm = d_tperm_.p; a.numSorted = numSorted_;
        a.numQueries = nq_; a.kcfg = cfg_.k;
        if (hits_) a.hits = hitList_.list();
        else {
            a.ed = d_mat_.p; a.nloc = d_mat_.p + cells_; a.end = d_mat_.p + 2 * cells_;
        }
        a.strand = !strands_ ? nullptr : (hits_ ? hitList_.byte.p : d_smat_.p);
        if (self_) {
            // (the condensed vector is one plane: numLocations and endLocation are 1 and length - 1 for NW)
            a.nloc = a.end = nullptr;
            a.qrank = g->d_rank.p; a.items = g->d_items.p; a.numItems = g->numItems;
            if (grouped_) {
                a.qend = g->d_end.p;
                EDLIB_AMD_HIP(launch_scan_cross_self_groups(g->words, syms_, a, stream_));
            } else
                EDLIB_AMD_HIP((strands_ ? launch_scan_cross_self_strands : launch_scan_cross_self)(g->words, syms_, hits_, a, stream_));
            if (g->numItems > 0) ++stats.scan_launches;
            stats.word_steps += g->wordSteps;
            continue;
        }
        if (occ_) EDLIB_AMD_HIP(launch_scan_cross_occ(g->words, syms_, a, g->ysplit, stream_));
        else
            EDLIB_AMD_HIP((strands_ ? launch_scan_cross_strands : launch_scan_cross)(g->words, syms_, (int)cfg_.mode, hits_, a,
                                                                                     g->ysplit, stream_));
        ++stats.scan_launches;
        stats.word_steps += g->wordSteps;
    }
    return 0;
}

// after the scans and the internal sessions: the list settled (a count past capacity grows it and scans again, so later
// Runs of the batch fit; the internal sessions' hits behind the kernel's) and finished on the device
int CrossBatch::finishHits()
{
    if (hitList_.settle(otherHits_, stream_, [&] { return scanGroups(); })) return 1;
    if (occ_) EDLIB_AMD_HIP(launch_cross_occ_finish(hitList_, nt_, stream_));
    else
        EDLIB_AMD_HIP(launch_cross_hits_finish(hitList_, nq_, nt_, d_bkey_.p, d_best_.p, strands_ ? d_sbest_.p : nullptr, stream_));
    return 0;
}

// occurrence batches: each target outside the kernel's envelope through its hit-list session; the session's runs (CSR by
// query, ascending firstEnd) re-keyed to the target's index, in that order behind what the last session left
int CrossBatch::runOccurrenceSessions()
{
    for (size_t s = 0; s < outShared_.size(); ++s) {
        Batch& b = *outShared_[s];
        if (b.run()) return 1;
        EdlibAmdReadHits rv{};
        if (b.hitsView(&rv)) return 1;
        const unsigned long long t = (unsigned long long)(uint32_t)outTargets_[s];
        for (int q = 0; q < rv.numUnits; ++q)
            for (long long i = rv.unitOffsets[q]; i < rv.unitOffsets[q + 1]; ++i) {
                otherHits_.key.push_back((t << 32) | (unsigned long long)(uint32_t)q);
                const int v[5] = {rv.firstEnd[i], rv.lastEnd[i], rv.editDistance[i], rv.endLocation[i], rv.numLocations[i]};
                for (int f = 0; f < 5; ++f) otherHits_.val[f].push_back(v[f]);
            }
        addSessionStats(b, true);
    }
    return 0;
}

int CrossBatch::run()
{
    if (self_) return runSelf();
    if (noTargets_) return noResults();
    pool_quarantine(false);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard guard(device_);
    if (beginRun(guard.status, {&mat_, &best_, &hitList_.result, &cellStrand_, &bestStrand_})) return 1;
    int* ed = d_mat_.p; int* nloc = hits_ ? nullptr : ed + cells_; int* end = hits_ ? nullptr : ed + 2 * cells_;
    if (hits_) EDLIB_AMD_HIP(hitList_.reset(stream_));

    // the cross kernel: Peq of every query, then one scan per word group
    if (scanRun(groups_, 8, [&] { return scanGroups(); })) return 1;
    // the other engines run on their own streams meanwhile
    otherHits_.clear();
    if (occ_ && runOccurrenceSessions()) return 1;
    if (otherCells_ > 0) {
        int* vals = reinterpret_cast<int*>(h_vals_.p);
        uint8_t* svals = strands_ ? h_svals_.p : nullptr;
        size_t at = 0;
        for (auto& b : outShared_) {
            if (b->run()) return 1;
            if (gather(*b, (size_t)nq_, vals + 3 * at, strands_ ? svals + at : nullptr)) return 1;
            at += (size_t)nq_;
            addSessionStats(*b, true);
        }
        if (longPairs_) {
            if (longPairs_->run()) return 1;
            if (!strands_) {
                if (gather(*longPairs_, longCells_.size(), vals + 3 * at, nullptr)) return 1;
            } else {
                // the pairs 2c (forward) and 2c + 1 (reverse complement) of every cell, decided here
                const size_t nc = longCells_.size();
                std::vector<int> both(6 * nc);
                if (gather(*longPairs_, 2 * nc, both.data(), nullptr)) return 1;
                for (size_t c = 0; c < nc; ++c) {
                    const int w = resolve_strands(both[6 * c], both[6 * c + 3]);
                    const int* rec = both.data() + 6 * c + ((w & kStrandReverse) ? 3 : 0);
                    for (int f = 0; f < 3; ++f) vals[3 * (at + c) + f] = rec[f];
                    svals[at + c] = (uint8_t)(w & (kStrandReverse | kStrandBoth));
                }
            }
            addSessionStats(*longPairs_, true);
        }
        if (!hits_) {
            EDLIB_AMD_HIP(hipMemcpyAsync(d_vals_.p, vals, 3 * (size_t)otherCells_ * sizeof(int), hipMemcpyHostToDevice, stream_));
            EDLIB_AMD_HIP(launch_cross_scatter(d_cells_.p, d_vals_.p, otherCells_, ed, nloc, end, stream_));
            if (strands_) {
                EDLIB_AMD_HIP(hipMemcpyAsync(d_svals_.p, svals, (size_t)otherCells_, hipMemcpyHostToDevice, stream_));
                EDLIB_AMD_HIP(launch_cross_scatter_bytes(d_cells_.p, d_svals_.p, otherCells_, d_smat_.p, stream_));
            }
        } else {
            // their cells within k: ed, nloc, end
            for (long long i = 0; i < otherCells_; ++i) {
                if (vals[3 * i] == -1) continue;
                const long long c = otherCellIdx_[(size_t)i];
                otherHits_.key.push_back(((unsigned long long)(c / nq_) << 32) | (unsigned long long)(c % nq_));
                for (int f = 0; f < 3; ++f) otherHits_.val[f].push_back(vals[3 * i + f]);
                if (strands_) otherHits_.byte.push_back(svals[i]);
            }
        }
    }
    if (hits_) {
        if (finishHits()) return 1;
    } else {
        int* bq = d_best_.p; int* bt = d_best_.p + 3 * (size_t)nt_;
        EDLIB_AMD_HIP(launch_cross_best(ed, nq_, nt_, bq, bq + nt_, bq + 2 * (size_t)nt_, bt, bt + nq_, bt + 2 * (size_t)nq_,
                                        d_partial_.p, targetChunk_, stream_));
        if (strands_) EDLIB_AMD_HIP(launch_cross_best_strands(d_smat_.p, nq_, nt_, bq, bt, d_sbest_.p, stream_));
    }
    return endRun(t0, !groups_.empty());
}

int CrossBatch::view(int what, EdlibAmdCrossView* out)
{
    if (occ_) { set_error("edlibAmdBatchCrossView: not available on an occurrence batch (edlibAmdBatchCrossOccurrences has its results)"); return 1; }
    if (!haveRun_) return noResults();
    if (what & ~(EDLIB_AMD_CROSS_MATRIX | EDLIB_AMD_CROSS_BEST)) { set_error("cross view: unknown parts %d", what); return 1; }
    if (hits_ && (what & EDLIB_AMD_CROSS_MATRIX)) {
        set_error("cross view: a hit-list batch keeps no matrix (edlibAmdBatchCrossHits has its cells within k; "
                  "create the batch with edlibAmdBatchCreateCross for EDLIB_AMD_CROSS_MATRIX)");
        return 1;
    }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t matBytes = 3 * cells_ * sizeof(int), bestBytes = (3 * (size_t)nt_ + 3 * (size_t)nq_) * sizeof(int);
    if (fetchParts({{what & EDLIB_AMD_CROSS_MATRIX, &mat_, d_mat_.p, matBytes},
                    {what & EDLIB_AMD_CROSS_BEST, &best_, d_best_.p, bestBytes}})) return 1;
    memset(out, 0, sizeof *out);
    out->numQueries = nq_; out->numTargets = nt_;
    if (what & EDLIB_AMD_CROSS_MATRIX) {
        const int* m = reinterpret_cast<const int*>(mat_.h.p);
        out->editDistance = m; out->numLocations = m + cells_; out->endLocation = m + 2 * cells_;
    }
    if (what & EDLIB_AMD_CROSS_BEST) {
        const int* b = reinterpret_cast<const int*>(best_.h.p);
        out->bestQuery = b; out->bestQueryDistance = b + nt_; out->secondQueryDistance = b + 2 * (size_t)nt_;
        b += 3 * (size_t)nt_;
        out->bestTarget = b; out->bestTargetDistance = b + nq_; out->secondTargetDistance = b + 2 * (size_t)nq_;
    }
    return 0;
}

int CrossBatch::hitsView(EdlibAmdCrossHits* out)
{
    if (occ_) { set_error("edlibAmdBatchCrossHits: not available on an occurrence batch (edlibAmdBatchCrossOccurrences has its results)"); return 1; }
    if (!hits_) {
        set_error("edlibAmdBatchCrossHits: not a hit-list batch (create it with edlibAmdBatchCreateCrossHits; a dense cross "
                  "batch has edlibAmdBatchCrossView)");
        return 1;
    }
    if (!haveRun_) return noResults();
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const int* l = nullptr;
    memset(out, 0, sizeof *out);
    if (hitList_.fetch(4, stream_, &out->targetOffsets, &l)) return 1;
    out->numQueries = nq_; out->numTargets = nt_; out->numHits = hitList_.outN;
    const size_t n = (size_t)hitList_.outN;
    out->query = l; out->editDistance = l + n; out->numLocations = l + 2 * n; out->endLocation = l + 3 * n;
    return 0;
}

int CrossBatch::occurrencesView(EdlibAmdCrossOccurrences* out)
{
    if (!occ_) {
        set_error("edlibAmdBatchCrossOccurrences: not an occurrence batch (create it with edlibAmdBatchCreateCrossOccurrences; "
                  "a hit-list cross batch has edlibAmdBatchCrossHits, a dense one edlibAmdBatchCrossView)");
        return 1;
    }
    if (!haveRun_) return noResults();
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const int* l = nullptr;
    memset(out, 0, sizeof *out);
    if (hitList_.fetch(6, stream_, &out->targetOffsets, &l)) return 1;
    out->numQueries = nq_; out->numTargets = nt_; out->numHits = hitList_.outN;
    const size_t n = (size_t)hitList_.outN;
    out->query = l; out->firstEnd = l + n; out->lastEnd = l + 2 * n; out->editDistance = l + 3 * n;
    out->endLocation = l + 4 * n; out->numLocations = l + 5 * n;
    return 0;
}

int CrossBatch::strandsView(int what, EdlibAmdCrossStrands* out)
{
    if (occ_) { set_error("edlibAmdBatchCrossStrands: not available on an occurrence batch (edlibAmdBatchCrossOccurrences has its results)"); return 1; }
    if (!strands_) {
        set_error("edlibAmdBatchCrossStrands: not a both-strand cross batch (create it with "
                  "edlibAmdBatchCreateCrossBothStrands or edlibAmdBatchCreateCrossHitsBothStrands)");
        return 1;
    }
    if (!haveRun_) return noResults();
    if (what & ~(EDLIB_AMD_CROSS_MATRIX | EDLIB_AMD_CROSS_BEST)) { set_error("cross strands: unknown parts %d", what); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t cellBytes = hits_ ? (size_t)hitList_.outN : cells_, bestBytes = (size_t)nt_ + (size_t)nq_;
    if (fetchParts({{what & EDLIB_AMD_CROSS_MATRIX, &cellStrand_, hits_ ? hitList_.byteOut.p : d_smat_.p, cellBytes},
                    {what & EDLIB_AMD_CROSS_BEST, &bestStrand_, d_sbest_.p, bestBytes}})) return 1;
    memset(out, 0, sizeof *out);
    out->numQueries = nq_; out->numTargets = nt_; out->numHits = hits_ ? hitList_.outN : 0;
    if (what & EDLIB_AMD_CROSS_MATRIX) (hits_ ? out->hitStrand : out->cellStrand) = cellStrand_.h.p;
    if (what & EDLIB_AMD_CROSS_BEST) { out->bestQueryStrand = bestStrand_.h.p; out->bestTargetStrand = bestStrand_.h.p + nt_; }
    return 0;
}

int CrossBatch::neighborsLevel(const char* who, int K, int maxDistance, int* level)
{
    if (K < 1 || K > 64) { set_error("%s: K must be 1..64 (got %d)", who, K); return 1; }
    if (cfg_.k >= 0 && maxDistance > cfg_.k) {
        set_error("%s: maxDistance %d is above the batch's k = %d: the batch kept nothing beyond k (create it with a "
                  "larger k)", who, maxDistance, cfg_.k);
        return 1;
    }
    // (< 0: every distance the batch reports -- an empty sequence's pairs are reported at the other's length whatever k,
    // and the nearest / best views count them: so do the neighbours)
    *level = maxDistance >= 0 ? maxDistance : -1;
    return 0;
}

int CrossBatch::selectNeighbors(const NeighborsSource& src, int K, int level, EdlibAmdNeighbors* out)
{
    const int rows = src.numRows;
    const size_t cells = (size_t)rows * (size_t)K;
    EDLIB_AMD_HIP(d_nbr_.ensure(NeighborsBuffers::ints(rows, K)));
    const NeighborsBuffers b = NeighborsBuffers::carve(d_nbr_.p, rows, K);
    EDLIB_AMD_HIP(launch_neighbors_select(src, K, level, b, stream_));
    // count, neighbor, distance and -- behind them on the device -- the strand bytes: one copy
    const size_t bytes = ((size_t)rows + 2 * cells) * sizeof(int) + (strands_ ? cells : 0);
    nbr_.fetched = false;
    EDLIB_AMD_HIP(nbr_.fetch(d_nbr_.p, bytes, stream_, 0, 4 * sizeof(int)));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    nbr_.fetched = true;
    const int* h = reinterpret_cast<const int*>(nbr_.h.p);
    memset(out, 0, sizeof *out);
    out->numRows = rows; out->K = K;
    out->count = h; out->neighbor = h + rows; out->distance = h + rows + cells;
    if (strands_) out->strand = reinterpret_cast<const unsigned char*>(h + rows + 2 * cells);
    return 0;
}

int CrossBatch::crossNeighbors(int K, int maxDistance, EdlibAmdNeighbors* out)
{
    int level = -1;
    if (occ_) {
        set_error("edlibAmdBatchCrossNeighbors: not available on an occurrence batch (its entries are runs of columns, not "
                  "cells: take edlibAmdBatchCrossOccurrences, or create a hit-list batch)");
        return 1;
    }
    if (!haveRun_) return noResults();
    if (neighborsLevel("cross neighbors", K, maxDistance, &level)) return 1;
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    NeighborsSource src{};
    src.numRows = nt_; src.rowLength = nq_;
    if (!hits_) {
        // row t of the matrix: the distances of its queries, the index implicit
        src.kind = NeighborsSource::kMatrix;
        src.ed = d_mat_.p;
        src.strand = strands_ ? d_smat_.p : nullptr;
    } else {
        // the finished list is the CSR by target itself: plane 0 the query, plane 1 the distance
        src.kind = NeighborsSource::kCsr;
        src.off = hitList_.off(); src.partner = hitList_.out(); src.distance = hitList_.out() + (size_t)hitList_.outN;
        src.strand = strands_ ? hitList_.byteOut.p : nullptr;
    }
    return selectNeighbors(src, K, level, out);
}

}  // namespace edlib_amd
