// engine_cross.hip -- host side of cross batches: every query against every target, DISTANCE only (DESIGN.md "Cross
// batches").  Create sorts the queries into word groups (kernel A's groups, each sorted by length) and the targets by
// length, packs the targets to 4-bit codes once and chooses each group's tile; a Run builds the Peq rows of every query
// (build_peq_reads_kernel over the union target alphabet), scans every group on the cross kernel, lets the internal
// sessions of the cells outside the kernel's envelope run meanwhile, scatters their results into the matrix and reduces
// it to the best hits.  Results stay in HBM until view() asks for a part of them.  A hit-list batch appends the cells
// within k instead (the scan, then the internal sessions' cells behind them) and finishes the list on the device
// (cross_hits.hip): sorted into CSR order, target offsets, best hits from the list.
// A both-strand batch makes the pool of every query and its reverse complement on the device, gives mates
// the slots s and s ^ 1 of their word group, and keeps a strand byte beside every cell, hit and best hit.
#include "engine.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace edlib_amd {

CrossBatch::~CrossBatch()
{
    DeviceGuard guard(device_);
    if (stream_) { (void)hipStreamSynchronize(stream_); pool_stream_release(stream_); }
}

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

int CrossBatch::init(const char* queries, const long long* qoffIn, int nq, const char* targets,
                     const long long* toffIn, int nt, EdlibAlignConfig cfg, int device, bool hits, bool strands)
{
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
    const int ndev = device_count();
    if (ndev == 0) { set_error("no usable HIP device (this library has no CPU fallback)"); return 1; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return 1; }
    cfg_ = cfg;
    if (cfg.additionalEqualities && cfg.additionalEqualitiesLength > 0)
        eqs_.assign(cfg.additionalEqualities, cfg.additionalEqualities + cfg.additionalEqualitiesLength);
    cfg_.additionalEqualities = eqs_.empty() ? nullptr : eqs_.data();
    cfg_.additionalEqualitiesLength = (int)eqs_.size();
    device_ = device; nq_ = nq; nt_ = nt; hits_ = hits; strands_ = strands;
    std::vector<long long> qoff(nq + 1, 0), toff(nt + 1, 0);
    if (nq > 0) qoff.assign(qoffIn, qoffIn + nq + 1);
    if (nt > 0) toff.assign(toffIn, toffIn + nt + 1);
    for (int i = 0; i < nq; ++i)
        if (qoff[i + 1] < qoff[i] || qoff[i + 1] - qoff[i] > 0x7fffffffLL) { set_error("bad query offsets"); return 1; }
    for (int i = 0; i < nt; ++i)
        if (toff[i + 1] < toff[i] || toff[i + 1] - toff[i] > 0x7fffffffLL) { set_error("bad target offsets"); return 1; }
    const long long qb = qoff[0], tb = toff[0];
    const long long qbytes = qoff[nq] - qb, tbytes = toff[nt] - tb;
    auto qlen = [&](int q) { return (int)(qoff[q + 1] - qoff[q]); };
    auto tlen = [&](int t) { return (int)(toff[t + 1] - toff[t]); };
    cells_ = (size_t)nq * (size_t)nt;
    stats = EdlibAmdBatchStats{};
    stats.cells = qbytes * tbytes * (strands ? 2 : 1);

    // the union alphabet of all targets decides the Peq rows (and whether the kernel can take any cell)
    build_tables(tab_, reinterpret_cast<const uint8_t*>(targets) + tb, tbytes, eqs_.data(), (int)eqs_.size());
    const bool wide = tab_.sigmaT > kCrossMaxSyms;
    syms_ = tab_.sigmaT <= 4 ? 4 : (tab_.sigmaT <= 8 ? 8 : 16);
    std::vector<int> inT, longQ;
    for (int t = 0; t < nt; ++t) {
        if (!wide && tlen(t) <= kCrossMaxTarget) inT.push_back(t);
        else outTargets_.push_back(t);
    }
    for (int q = 0; q < nq; ++q)
        if (qlen(q) > 32 * kCrossMaxQueryWords) longQ.push_back(q);

    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    EDLIB_AMD_HIP(pool_stream(&stream_));
    EDLIB_AMD_HIP(evScan0_.create()); EDLIB_AMD_HIP(evScan1_.create());
    EDLIB_AMD_HIP(d_best_.alloc(3 * (size_t)nt + 3 * (size_t)nq));
    if (strands_) {
        EDLIB_AMD_HIP(d_sbest_.alloc(std::max<size_t>((size_t)nt + (size_t)nq, 1)));
        if (!hits_) EDLIB_AMD_HIP(d_smat_.alloc(std::max<size_t>(cells_, 1)));
    }
    if (!hits_) {
        EDLIB_AMD_HIP(d_mat_.alloc(3 * std::max<size_t>(cells_, 1)));
        targetChunk_ = std::max(1024, (nt + 32767) / 32768);
        EDLIB_AMD_HIP(d_partial_.alloc((size_t)std::max(1, (nt + targetChunk_ - 1) / targetChunk_) * (size_t)std::max(nq, 1)));
    } else {
        EDLIB_AMD_HIP(d_hcount_.alloc(1)); EDLIB_AMD_HIP(h_hcount_.alloc(sizeof(unsigned long long)));
        EDLIB_AMD_HIP(d_htoff_.alloc((size_t)nt + 1));
        EDLIB_AMD_HIP(d_bkey_.alloc(2 * ((size_t)nt + (size_t)nq)));
        if (growHits(std::max<long long>(1LL << 20, (long long)nq + nt))) return 1;
    }

    // ---- the cross kernel's share
    if (!inT.empty() && (int)longQ.size() < nq) {
        std::stable_sort(inT.begin(), inT.end(), [&](int a, int b) { return tlen(a) < tlen(b); });
        numSorted_ = (int)inT.size();
        std::vector<long long> tdw(numSorted_), colsBelow(numSorted_ + 1, 0);
        std::vector<int> tl(numSorted_);
        long long dw = 0;
        for (int i = 0; i < numSorted_; ++i) {
            tdw[i] = dw; tl[i] = tlen(inT[i]);
            dw += (tl[i] + 7) / 8;
            sortedCols_ += tl[i];
            colsBelow[i + 1] = sortedCols_;
        }
        // columns the kernel scans for a query of length m: all of them, or under NW with k >= 0 those of the targets in
        // the length window [m - k, m + k] (cross_nw_outside), a range of the sorted lengths
        auto scannedCols = [&](int m) -> long long {
            if (cfg.mode == EDLIB_MODE_NW && cfg.k >= 0) {
                const long long lo = std::lower_bound(tl.begin(), tl.end(), (long long)m - cfg.k) - tl.begin();
                const long long hi = std::upper_bound(tl.begin(), tl.end(), (long long)m + cfg.k) - tl.begin();
                return colsBelow[hi] - colsBelow[lo];
            }
            return sortedCols_;
        };
        EDLIB_AMD_HIP(d_tpk_.alloc((size_t)std::max(dw, 1LL)));
        EDLIB_AMD_HIP(d_tdw_.alloc(numSorted_)); EDLIB_AMD_HIP(d_tlen_.alloc(numSorted_)); EDLIB_AMD_HIP(d_tperm_.alloc(numSorted_));
        EDLIB_AMD_HIP(hipMemcpy(d_tdw_.p, tdw.data(), numSorted_ * sizeof(long long), hipMemcpyHostToDevice));
        EDLIB_AMD_HIP(hipMemcpy(d_tlen_.p, tl.data(), numSorted_ * sizeof(int), hipMemcpyHostToDevice));
        EDLIB_AMD_HIP(hipMemcpy(d_tperm_.p, inT.data(), numSorted_ * sizeof(int), hipMemcpyHostToDevice));
        {   // the raw target pool is only needed by the pack
            DevBuf<uint8_t> d_traw, d_tlut; DevBuf<long long> d_toff;
            std::vector<long long> toffR(toff);
            for (auto& v : toffR) v -= tb;
            EDLIB_AMD_HIP(d_traw.alloc((size_t)tbytes + 16)); EDLIB_AMD_HIP(d_tlut.alloc(256)); EDLIB_AMD_HIP(d_toff.alloc(nt + 1));
            if (tbytes) EDLIB_AMD_HIP(hipMemcpy(d_traw.p, targets + tb, (size_t)tbytes, hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(d_tlut.p, tab_.tlut, 256, hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(d_toff.p, toffR.data(), (nt + 1) * sizeof(long long), hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(launch_pack_cross_targets(d_traw.p, d_toff.p, d_tperm_.p, d_tdw_.p, numSorted_, d_tlut.p, d_tpk_.p, stream_));
            EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        }
        // queries (rebased), their tables
        std::vector<long long> qoffR(qoff);
        for (auto& v : qoffR) v -= qb;
        if (!strands_) {
            EDLIB_AMD_HIP(d_qpool_.alloc((size_t)qbytes + 16)); EDLIB_AMD_HIP(d_qoff_.alloc(nq + 1));
            if (qbytes) EDLIB_AMD_HIP(hipMemcpy(d_qpool_.p, queries + qb, (size_t)qbytes, hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(d_qoff_.p, qoffR.data(), (nq + 1) * sizeof(long long), hipMemcpyHostToDevice));
        } else {
            // the caller's pool goes up as it is; query i and its reverse complement are written from it on the device as
            // the entries 2i and 2i + 1 of a pool twice its size
            if (make_strand_pool(queries + qb, qoffR.data(), nq, d_qpool_, d_qoff_, stream_)) return 1;
        }
        EDLIB_AMD_HIP(d_eqtbl_.alloc(256)); EDLIB_AMD_HIP(d_presence_.alloc(8));
        EDLIB_AMD_HIP(hipMemcpy(d_eqtbl_.p, tab_.eqtbl, 512, hipMemcpyHostToDevice));
        EDLIB_AMD_HIP(hipMemcpy(d_presence_.p, tab_.presence, 32, hipMemcpyHostToDevice));
        // word groups, each sorted by length; empty queries ride in the one-word group
        std::vector<std::vector<int>> byWords(kCrossMaxQueryWords + 1);
        for (int q = 0; q < nq; ++q) {
            const int m = qlen(q);
            if (m > 32 * kCrossMaxQueryWords) continue;
            byWords[std::max(1, (m + 31) / 32)].push_back(q);
        }
        for (int w = 1; w <= kCrossMaxQueryWords; ++w) {
            auto& qs = byWords[w];
            if (qs.empty()) continue;
            std::stable_sort(qs.begin(), qs.end(), [&](int a, int b) { return qlen(a) < qlen(b); });
            std::unique_ptr<Group> g(new Group);
            g->words = w;
            // both strands: each query of the sorted list becomes two slots, itself and its reverse complement
            const long long need = (long long)qs.size() * (strands_ ? 2 : 1);
            g->qt = choose_qt(need, numSorted_, strands_ ? 2 : 1);
            g->tiles = (int)((need + g->qt - 1) / g->qt);
            g->slots = g->tiles * g->qt;
            for (int q : qs) g->wordSteps += (long long)w * scannedCols(qlen(q)) * (strands_ ? 2 : 1);
            const int tpt = 64 / g->qt;
            const long long targetTiles = (numSorted_ + tpt - 1) / tpt;
            // about 8,192 waves per launch (256 CUs), each persistent over a strided range of target tiles
            g->ysplit = (int)std::min<long long>({targetTiles, std::max(1LL, (8192LL + g->tiles - 1) / g->tiles), 65535LL});
            std::vector<int> perm(g->slots, -1);
            if (!strands_) std::copy(qs.begin(), qs.end(), perm.begin());
            else {
                for (size_t i = 0; i < qs.size(); ++i) { perm[2 * i] = 2 * qs[i]; perm[2 * i + 1] = 2 * qs[i] + 1; }
                // what the kernel's lane exchange rests on: mates in the slots s and s ^ 1, padding in pairs, an even tile
                bool ok = !(g->qt & 1) && !(g->slots & 1);
                for (int sl = 0; ok && sl < g->slots; sl += 2)
                    ok = perm[sl] < 0 ? perm[sl + 1] < 0 : (!(perm[sl] & 1) && perm[sl + 1] == perm[sl] + 1);
                if (!ok) { set_error("both strands: mates are not in adjacent slots"); return 1; }
            }
            const size_t blocks = (size_t)(g->slots + 63) / 64;
            EDLIB_AMD_HIP(g->d_perm.alloc(g->slots)); EDLIB_AMD_HIP(g->d_qlen.alloc(g->slots));
            EDLIB_AMD_HIP(g->d_kinit.alloc(g->slots)); EDLIB_AMD_HIP(g->d_alpha.alloc(g->slots));
            EDLIB_AMD_HIP(g->d_peq.alloc(blocks * syms_ * w * 64));
            EDLIB_AMD_HIP(hipMemcpy(g->d_perm.p, perm.data(), g->slots * sizeof(int), hipMemcpyHostToDevice));
            groups_.push_back(std::move(g));
        }
    }

    // ---- the other engines' share
    if (nq > 0) {
        for (int t : outTargets_) {
            std::unique_ptr<Batch> b(new Batch);
            const long long to[2] = {toff[t], toff[t + 1]};
            if (b->init(queries, qoffIn, nq, targets, to, 1, cfg_, device, strands_)) return 1;
            outShared_.push_back(std::move(b));
            otherCells_ += nq;
        }
        if (!longQ.empty() && !inT.empty()) {
            // every long query against every target the kernel takes, as pairs (their bytes replicated per cell)
            std::vector<char> qp, tp;
            std::vector<long long> qo(1, 0), to(1, 0);
            // (both strands: the pairs 2c and 2c + 1 of cell c, the second with the reverse complement made here)
            for (int t : inT)
                for (int q : longQ) {
                    for (int st = 0; st < (strands_ ? 2 : 1); ++st) {
                        if (!st) qp.insert(qp.end(), queries + qoff[q], queries + qoff[q + 1]);
                        else
                            for (long long j = qoff[q + 1] - 1; j >= qoff[q]; --j)
                                qp.push_back((char)complement_byte((uint8_t)queries[j]));
                        tp.insert(tp.end(), targets + toff[t], targets + toff[t + 1]);
                        qo.push_back((long long)qp.size()); to.push_back((long long)tp.size());
                    }
                    longCells_.push_back((long long)t * nq + q);
                }
            const long long np = (long long)longCells_.size() * (strands_ ? 2 : 1);
            if (np > 0x7fffffffLL) { set_error("cross batch: too many cells of long queries (%lld pairs)", np); return 1; }
            if (tp.empty()) tp.push_back(0);
            longPairs_.reset(new Batch);
            if (longPairs_->init(qp.data(), qo.data(), (int)np, tp.data(), to.data(), (int)np, cfg_, device)) return 1;
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

// editDistance / numLocations / first end location of the n units of an internal session's last run; sbytes (a both-strand
// session): their strand bytes
int CrossBatch::gather(Batch& b, size_t n, int* vals, uint8_t* sbytes)
{
    EdlibAmdResultsView v{};
    if (b.resultsView(&v)) return 1;
    if (sbytes) {
        EdlibAmdStrandView sv{};
        if (b.strandView(&sv)) return 1;
        for (size_t i = 0; i < n; ++i)
            sbytes[i] = v.editDistance[i] < 0 ? 0 : (uint8_t)((sv.strand[i] ? kStrandReverse : 0) | (sv.bothStrands[i] ? kStrandBoth : 0));
    }
    for (size_t i = 0; i < n; ++i) {
        if (v.status[i] != EDLIB_STATUS_OK) { set_error("cross batch: an internal alignment failed"); return 1; }
        vals[3 * i] = v.editDistance[i];
        vals[3 * i + 1] = v.numLocations[i];
        vals[3 * i + 2] = v.numLocations[i] > 0 ? v.endLocations[v.locOffsets[i]] : -1;
    }
    return 0;
}

// one scan per word group (the Peq is built); a hit-list batch counts its hits from 0
int CrossBatch::scanGroups()
{
    if (hits_) EDLIB_AMD_HIP(hipMemsetAsync(d_hcount_.p, 0, sizeof(unsigned long long), stream_));
    for (auto& g : groups_) {
        CrossScanArgs a{};
        a.peq = g->d_peq.p; a.qlen = g->d_qlen.p; a.qperm = g->d_perm.p; a.qt = g->qt; a.numQueryTiles = g->tiles;
        a.tpk = d_tpk_.p; a.tdw = d_tdw_.p; a.tlen = d_tlen_.p; a.tperm = d_tperm_.p; a.numSorted = numSorted_;
        a.numQueries = nq_; a.kcfg = cfg_.k;
        if (hits_) {
            a.hitCount = d_hcount_.p; a.hitCap = (unsigned long long)hitCap_; a.hitKey = d_hkey_.p; a.hitVal = d_hval_.p;
        } else {
            a.ed = d_mat_.p; a.nloc = d_mat_.p + cells_; a.end = d_mat_.p + 2 * cells_;
        }
        a.strand = !strands_ ? nullptr : (hits_ ? d_hstrand_.p : d_smat_.p);
        if (self_) {
            // (the condensed vector is one plane: numLocations and endLocation are 1 and length - 1 for NW)
            a.nloc = a.end = nullptr;
            a.qrank = g->d_rank.p; a.items = g->d_items.p; a.numItems = g->numItems;
            EDLIB_AMD_HIP(launch_scan_cross_self(g->words, syms_, hits_, a, stream_));
            if (g->numItems > 0) ++stats.scan_launches;
            stats.word_steps += g->wordSteps;
            continue;
        }
        EDLIB_AMD_HIP((strands_ ? launch_scan_cross_strands : launch_scan_cross)(g->words, syms_, (int)cfg_.mode, hits_, a,
                                                                                 g->ysplit, stream_));
        ++stats.scan_launches;
        stats.word_steps += g->wordSteps;
    }
    return 0;
}

// the hit list and its sort / CSR buffers for `cap` hits (what they held is gone)
int CrossBatch::growHits(long long cap)
{
    hitCap_ = 0;
    size_t tmp = 0;
    hipError_t e = d_hkey_.alloc((size_t)cap);
    if (e == hipSuccess) e = d_hval_.alloc(3 * (size_t)cap);
    if (e == hipSuccess) e = d_hidx_.alloc((size_t)cap);
    if (e == hipSuccess) e = d_skey_.alloc((size_t)cap);
    if (e == hipSuccess) e = d_sidx_.alloc((size_t)cap);
    if (e == hipSuccess) e = d_hout_.alloc(4 * (size_t)cap);
    if (e == hipSuccess && strands_) e = d_hstrand_.alloc((size_t)cap);
    if (e == hipSuccess && strands_) e = d_hsout_.alloc((size_t)cap);
    if (e == hipSuccess) e = cross_hits_sort_bytes(cap, nt_, &tmp);
    if (e == hipSuccess) e = d_sortTmp_.alloc(tmp);
    if (e == hipSuccess) e = launch_cross_hits_iota(d_hidx_.p, cap, stream_);
    if (e != hipSuccess) {
        set_error("cross batch: no room on the device for a hit list of %lld hits (%s)", cap, hipGetErrorString(e));
        return 1;
    }
    hitCap_ = cap;
    return 0;
}

// after the scans and the internal sessions: the kernel's count (the sort needs it anyway); a count past capacity grows
// the list to it and scans again, so later Runs of the batch fit.  Then the internal sessions' hits behind the kernel's,
// and the list finished on the device.
int CrossBatch::finishHits()
{
    unsigned long long* hc = reinterpret_cast<unsigned long long*>(h_hcount_.p);
    EDLIB_AMD_HIP(hipMemcpyAsync(hc, d_hcount_.p, sizeof *hc, hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    const long long kernelHits = (long long)*hc, extra = (long long)xKey_.size(), total = kernelHits + extra;
    if (total > 0xffffffffLL) {
        set_error("cross batch: %lld hits, more than a hit list holds (2^32 - 1): lower k or split the batch", total);
        return 1;
    }
    if (total > hitCap_) {
        if (growHits(total)) return 1;
        if (kernelHits > 0 && scanGroups()) return 1;
    }
    if (extra > 0) {
        const size_t cap = (size_t)hitCap_;
        EDLIB_AMD_HIP(hipMemcpyAsync(d_hkey_.p + kernelHits, xKey_.data(), (size_t)extra * sizeof(unsigned long long),
                                     hipMemcpyHostToDevice, stream_));
        for (int f = 0; f < 3; ++f)
            EDLIB_AMD_HIP(hipMemcpyAsync(d_hval_.p + f * cap + kernelHits, xVal_.data() + f * (size_t)extra,
                                         (size_t)extra * sizeof(int), hipMemcpyHostToDevice, stream_));
        if (strands_)
            EDLIB_AMD_HIP(hipMemcpyAsync(d_hstrand_.p + kernelHits, xStrand_.data(), (size_t)extra, hipMemcpyHostToDevice, stream_));
    }
    size_t tmp = 0;
    EDLIB_AMD_HIP(cross_hits_sort_bytes(total, nt_, &tmp));
    if (tmp > d_sortTmp_.n) EDLIB_AMD_HIP(d_sortTmp_.alloc(tmp));
    EDLIB_AMD_HIP(launch_cross_hits_finish(d_hkey_.p, d_hval_.p, hitCap_, total, nq_, nt_, d_hidx_.p, d_skey_.p, d_sidx_.p,
                                           d_sortTmp_.p, d_sortTmp_.n, d_htoff_.p, d_hout_.p, d_bkey_.p, d_best_.p,
                                           strands_ ? d_hstrand_.p : nullptr, d_hsout_.p, d_sbest_.p, stream_));
    numHits_ = total;
    return 0;
}

int CrossBatch::run()
{
    if (self_) return runSelf();
    pool_quarantine(false);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    haveRun_ = matFetched_ = bestFetched_ = hitsFetched_ = cellStrandFetched_ = bestStrandFetched_ = false;
    const long long cells = stats.cells;
    stats = EdlibAmdBatchStats{};
    stats.cells = cells;
    int* ed = d_mat_.p; int* nloc = hits_ ? nullptr : ed + cells_; int* end = hits_ ? nullptr : ed + 2 * cells_;
    if (hits_) EDLIB_AMD_HIP(hipMemsetAsync(d_hcount_.p, 0, sizeof(unsigned long long), stream_));

    // the cross kernel: Peq of every query, then one scan per word group
    if (!groups_.empty()) {
        for (auto& g : groups_)
            EDLIB_AMD_HIP(launch_build_peq_reads(g->words, syms_, d_qpool_.p, d_qoff_.p, g->d_perm.p, g->slots, d_eqtbl_.p,
                                                 d_presence_.p, cfg_.k, g->d_peq.p, g->d_qlen.p, g->d_kinit.p, g->d_alpha.p,
                                                 stream_));
        EDLIB_AMD_HIP(hipEventRecord(evScan0_.e, stream_));
        if (scanGroups()) return 1;
        EDLIB_AMD_HIP(hipEventRecord(evScan1_.e, stream_));
        stats.path |= 8;
    }
    // the other engines run on their own streams meanwhile
    xKey_.clear(); xVal_.clear(); xStrand_.clear();
    if (otherCells_ > 0) {
        int* vals = reinterpret_cast<int*>(h_vals_.p);
        uint8_t* svals = strands_ ? h_svals_.p : nullptr;
        size_t at = 0;
        for (auto& b : outShared_) {
            if (b->run()) return 1;
            if (gather(*b, (size_t)nq_, vals + 3 * at, strands_ ? svals + at : nullptr)) return 1;
            at += (size_t)nq_;
            b->finishStats();
            stats.word_steps += b->stats.word_steps; stats.scan_launches += b->stats.scan_launches;
            stats.path |= b->stats.path; stats.overflow_units += b->stats.overflow_units; stats.wide_retries += b->stats.wide_retries;
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
            longPairs_->finishStats();
            const EdlibAmdBatchStats& s = longPairs_->stats;
            stats.word_steps += s.word_steps; stats.scan_launches += s.scan_launches;
            stats.path |= s.path; stats.overflow_units += s.overflow_units; stats.wide_retries += s.wide_retries;
        }
        if (!hits_) {
            EDLIB_AMD_HIP(hipMemcpyAsync(d_vals_.p, vals, 3 * (size_t)otherCells_ * sizeof(int), hipMemcpyHostToDevice, stream_));
            EDLIB_AMD_HIP(launch_cross_scatter(d_cells_.p, d_vals_.p, otherCells_, ed, nloc, end, stream_));
            if (strands_) {
                EDLIB_AMD_HIP(hipMemcpyAsync(d_svals_.p, svals, (size_t)otherCells_, hipMemcpyHostToDevice, stream_));
                EDLIB_AMD_HIP(launch_cross_scatter_bytes(d_cells_.p, d_svals_.p, otherCells_, d_smat_.p, stream_));
            }
        } else {
            // their cells within k, as [key], [ed][nloc][end]
            std::vector<int> e3[3];
            for (long long i = 0; i < otherCells_; ++i) {
                if (vals[3 * i] == -1) continue;
                const long long c = otherCellIdx_[(size_t)i];
                xKey_.push_back(((unsigned long long)(c / nq_) << 32) | (unsigned long long)(c % nq_));
                for (int f = 0; f < 3; ++f) e3[f].push_back(vals[3 * i + f]);
                if (strands_) xStrand_.push_back(svals[i]);
            }
            for (int f = 0; f < 3; ++f) xVal_.insert(xVal_.end(), e3[f].begin(), e3[f].end());
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
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    if (!groups_.empty()) {
        float ms = 0.f;
        EDLIB_AMD_HIP(hipEventElapsedTime(&ms, evScan0_.e, evScan1_.e));
        stats.scan_ms = ms;
    }
    stats.algo_bytes = 0;
    stats.run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    haveRun_ = true;
    return 0;
}

int CrossBatch::view(int what, EdlibAmdCrossView* out)
{
    if (!haveRun_) { set_error("cross batch: no results (Run it first)"); return 1; }
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
    if ((what & EDLIB_AMD_CROSS_MATRIX) && !matFetched_) {
        if (h_mat_.n < matBytes || !h_mat_.p) EDLIB_AMD_HIP(h_mat_.alloc(matBytes));
        if (matBytes) EDLIB_AMD_HIP(hipMemcpyAsync(h_mat_.p, d_mat_.p, matBytes, hipMemcpyDeviceToHost, stream_));
    }
    if ((what & EDLIB_AMD_CROSS_BEST) && !bestFetched_) {
        if (h_best_.n < bestBytes || !h_best_.p) EDLIB_AMD_HIP(h_best_.alloc(bestBytes));
        if (bestBytes) EDLIB_AMD_HIP(hipMemcpyAsync(h_best_.p, d_best_.p, bestBytes, hipMemcpyDeviceToHost, stream_));
    }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    if (what & EDLIB_AMD_CROSS_MATRIX) matFetched_ = true;
    if (what & EDLIB_AMD_CROSS_BEST) bestFetched_ = true;
    memset(out, 0, sizeof *out);
    out->numQueries = nq_; out->numTargets = nt_;
    if (what & EDLIB_AMD_CROSS_MATRIX) {
        const int* m = reinterpret_cast<const int*>(h_mat_.p);
        out->editDistance = m; out->numLocations = m + cells_; out->endLocation = m + 2 * cells_;
    }
    if (what & EDLIB_AMD_CROSS_BEST) {
        const int* b = reinterpret_cast<const int*>(h_best_.p);
        out->bestQuery = b; out->bestQueryDistance = b + nt_; out->secondQueryDistance = b + 2 * (size_t)nt_;
        b += 3 * (size_t)nt_;
        out->bestTarget = b; out->bestTargetDistance = b + nq_; out->secondTargetDistance = b + 2 * (size_t)nq_;
    }
    return 0;
}

int CrossBatch::hitsView(EdlibAmdCrossHits* out)
{
    if (!hits_) {
        set_error("edlibAmdBatchCrossHits: not a hit-list batch (create it with edlibAmdBatchCreateCrossHits; a dense cross "
                  "batch has edlibAmdBatchCrossView)");
        return 1;
    }
    if (!haveRun_) { set_error("cross batch: no results (Run it first)"); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t offBytes = ((size_t)nt_ + 1) * sizeof(long long), listBytes = 4 * (size_t)numHits_ * sizeof(int);
    if (!hitsFetched_) {
        if (h_hits_.n < offBytes + listBytes || !h_hits_.p) EDLIB_AMD_HIP(h_hits_.alloc(offBytes + listBytes));
        EDLIB_AMD_HIP(hipMemcpyAsync(h_hits_.p, d_htoff_.p, offBytes, hipMemcpyDeviceToHost, stream_));
        if (listBytes)
            EDLIB_AMD_HIP(hipMemcpyAsync(h_hits_.p + offBytes, d_hout_.p, listBytes, hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        hitsFetched_ = true;
    }
    memset(out, 0, sizeof *out);
    out->numQueries = nq_; out->numTargets = nt_; out->numHits = numHits_;
    out->targetOffsets = reinterpret_cast<const long long*>(h_hits_.p);
    const int* l = reinterpret_cast<const int*>(h_hits_.p + offBytes);
    const size_t n = (size_t)numHits_;
    out->query = l; out->editDistance = l + n; out->numLocations = l + 2 * n; out->endLocation = l + 3 * n;
    return 0;
}

int CrossBatch::strandsView(int what, EdlibAmdCrossStrands* out)
{
    if (!strands_) {
        set_error("edlibAmdBatchCrossStrands: not a both-strand cross batch (create it with "
                  "edlibAmdBatchCreateCrossBothStrands or edlibAmdBatchCreateCrossHitsBothStrands)");
        return 1;
    }
    if (!haveRun_) { set_error("cross batch: no results (Run it first)"); return 1; }
    if (what & ~(EDLIB_AMD_CROSS_MATRIX | EDLIB_AMD_CROSS_BEST)) { set_error("cross strands: unknown parts %d", what); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t cellBytes = hits_ ? (size_t)numHits_ : cells_, bestBytes = (size_t)nt_ + (size_t)nq_;
    if ((what & EDLIB_AMD_CROSS_MATRIX) && !cellStrandFetched_) {
        if (h_smat_.n < cellBytes || !h_smat_.p) EDLIB_AMD_HIP(h_smat_.alloc(std::max<size_t>(cellBytes, 1)));
        if (cellBytes)
            EDLIB_AMD_HIP(hipMemcpyAsync(h_smat_.p, hits_ ? d_hsout_.p : d_smat_.p, cellBytes, hipMemcpyDeviceToHost, stream_));
    }
    if ((what & EDLIB_AMD_CROSS_BEST) && !bestStrandFetched_) {
        if (h_sbest_.n < bestBytes || !h_sbest_.p) EDLIB_AMD_HIP(h_sbest_.alloc(std::max<size_t>(bestBytes, 1)));
        if (bestBytes) EDLIB_AMD_HIP(hipMemcpyAsync(h_sbest_.p, d_sbest_.p, bestBytes, hipMemcpyDeviceToHost, stream_));
    }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    if (what & EDLIB_AMD_CROSS_MATRIX) cellStrandFetched_ = true;
    if (what & EDLIB_AMD_CROSS_BEST) bestStrandFetched_ = true;
    memset(out, 0, sizeof *out);
    out->numQueries = nq_; out->numTargets = nt_; out->numHits = hits_ ? numHits_ : 0;
    if (what & EDLIB_AMD_CROSS_MATRIX) (hits_ ? out->hitStrand : out->cellStrand) = h_smat_.p;
    if (what & EDLIB_AMD_CROSS_BEST) { out->bestQueryStrand = h_sbest_.p; out->bestTargetStrand = h_sbest_.p + nt_; }
    return 0;
}

}  // namespace edlib_amd
