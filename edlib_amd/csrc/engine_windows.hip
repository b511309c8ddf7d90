// engine_windows.hip -- host side of window batches: units over one resident target, unit u = query unitQuery[u] against
// the window [unitStart[u], unitStart[u] + unitLength[u]), DISTANCE only (DESIGN.md "Window batches").  Create checks the
// unit list and packs the target to 4-bit codes once.  A list inside the window kernel's envelope goes up as it is and
// the device sorts the queries into word groups (a cross batch's) and every group's units by window length
// (prepareUnits, window_units.hip); setUnits passes the next list through the resident batch the same way.  A list with
// units outside the envelope is grouped and sorted by the host, which sends those units to an internal pair session.
// Either way a unit has its query slot, start, length and place in the caller's order; nothing is sized by bytes of
// windows.  A Run builds the Peq rows of every query, scans every group on the window kernel, lets the
// internal pair session of the units outside the kernel's envelope run meanwhile, scatters its results into the unit
// arrays and reduces them to the best unit per query.  Results stay in HBM until view() asks for a part of them.
// Units with a strand: where a unit names the reverse complement of its query the query pool holds both
// strands of every query, made on the device (entry 2 q + strand), and a Peq slot goes to each (query, strand) a kernel
// unit names; the scan and the best reduction do not know about strands.
#include "engine_lanes.hpp"

#include <algorithm>
#include <cstring>

namespace edlib_amd {

int WindowBatch::checkUnits(const long long* qoff, int nq, int targetLength, const int* unitQuery, const int* unitStart,
                            const int* unitLength, const unsigned char* unitStrand, int nu, int mode, int k, UnitCensus& c)
{
    for (int u = 0; u < nu; ++u) {
        const int q = unitQuery[u], n = unitLength[u];
        if (q < 0 || q >= nq) {
            set_error("window batch: unit %d names query %d, outside [0, numQueries = %d)", u, q, nq);
            return 1;
        }
        if (unitStart[u] < 0) { set_error("window batch: unit %d has a negative unitStart (%d)", u, unitStart[u]); return 1; }
        if (n < 0) { set_error("window batch: unit %d has a negative unitLength (%d)", u, n); return 1; }
        if ((long long)unitStart[u] + (long long)n > (long long)targetLength) {
            set_error("window batch: unit %d ends past the target (unitStart %d + unitLength %d > targetLength %d)", u,
                      unitStart[u], n, targetLength);
            return 1;
        }
        if (unitStrand && unitStrand[u] > 1) {
            set_error("window batch: unit %d has unitStrand %d (0: the query, 1: its reverse complement)", u, (int)unitStrand[u]);
            return 1;
        }
        if (unitStrand && unitStrand[u]) c.stranded = true;
        const long long m = qoff[q + 1] - qoff[q];
        c.cells += m * n;
        if (m > 32 * kCrossMaxQueryWords || n > kCrossMaxTarget) {
            c.inside = false;
            if (n > kCrossMaxTarget && c.longUnit < 0) c.longUnit = u;
            continue;
        }
        const int w = std::max(1, ((int)m + 31) / 32);                    // empty queries ride in the one-word group
        ++c.units[w];
        if (m > 0 && n > 0 && !cross_nw_outside(mode, k, (int)m, n)) c.wordSteps[w] += (long long)w * n;
    }
    return 0;
}

int WindowBatch::init(const char* queries, const long long* qoffIn, int nq, const char* target, int targetLength,
                      const int* unitQuery, const int* unitStart, const int* unitLength, const unsigned char* unitStrand,
                      int nu, EdlibAlignConfig cfg, int device)
{
    // ---- refusals, before the device is looked at
    if (cfg.task != EDLIB_TASK_DISTANCE) {
        set_error("window batches compute distances only (EDLIB_TASK_DISTANCE): align the chosen units with a pair batch "
                  "for locations or paths");
        return 1;
    }
    if (cfg.mode != EDLIB_MODE_NW && cfg.mode != EDLIB_MODE_SHW && cfg.mode != EDLIB_MODE_HW) { set_error("unknown mode"); return 1; }
    if (nu < 0) { set_error("window batch: numUnits %d is negative", nu); return 1; }
    if (targetLength < 0) { set_error("negative target length"); return 1; }
    if (nq < 0 || (nq > 0 && !qoffIn) || (nu > 0 && (!unitQuery || !unitStart || !unitLength))) {
        set_error("bad batch shape");
        return 1;
    }
    std::vector<long long> qoff;
    if (copy_offsets(qoffIn, nq, "query", qoff)) return 1;
    UnitCensus census;
    if (checkUnits(qoff.data(), nq, targetLength, unitQuery, unitStart, unitLength, unitStrand, nu, (int)cfg.mode, cfg.k,
                   census)) return 1;
    const bool stranded = census.stranded;                                // a unit names a reverse complement
    if (stranded && nq > 0x3fffffff) { set_error("bad batch shape"); return 1; }
    auto strandOf = [&](int u) { return stranded ? (int)unitStrand[u] : 0; };
    if (check_device(device)) return 1;

    keep_config(cfg, cfg_, eqs_);
    device_ = device; nq_ = nq; nu_ = nu; targetLength_ = targetLength;
    auto qlen = [&](int q) { return (int)(qoff[q + 1] - qoff[q]); };
    stats = EdlibAmdBatchStats{};
    stats.cells = census.cells;

    build_tables(tab_, reinterpret_cast<const uint8_t*>(target), targetLength, eqs_.data(), (int)eqs_.size());
    const bool wide = tab_.sigmaT > kCrossMaxSyms;
    syms_ = peq_syms(tab_.sigmaT);
    auto onKernel = [&](int u) {
        return !wide && qlen(unitQuery[u]) <= 32 * kCrossMaxQueryWords && unitLength[u] <= kCrossMaxTarget;
    };

    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    if (openStream()) return 1;
    if (!wide) {
        // the target the window kernel can take is resident whatever this unit list leaves it (a later setUnits finds
        // it): 4-bit codes from dword 0, and the tables of its symbols
        if (packHostTargets(target, {0, targetLength}, {0}, {targetLength})) return 1;
        EDLIB_AMD_HIP(d_eqtbl_.ensure(256)); EDLIB_AMD_HIP(d_presence_.ensure(8));
        EDLIB_AMD_HIP(hipMemcpy(d_eqtbl_.p, tab_.eqtbl, 512, hipMemcpyHostToDevice));
        EDLIB_AMD_HIP(hipMemcpy(d_presence_.p, tab_.presence, 32, hipMemcpyHostToDevice));
        // a list that lies inside the kernel's envelope is prepared on the device, the way setUnits does it; one with a
        // unit outside it takes the host loop below, where the pair route changes the kernel's subset
        if (census.inside)
            return prepareUnits(queries, qoff.data(), nq, unitQuery, unitStart, unitLength, unitStrand, nu, census);
    }
    EDLIB_AMD_HIP(d_units_.alloc(3 * (size_t)std::max(nu, 1)));
    EDLIB_AMD_HIP(d_uq_.alloc((size_t)std::max(nu, 1)));
    EDLIB_AMD_HIP(d_best_.alloc(3 * (size_t)std::max(nq, 1)));
    EDLIB_AMD_HIP(d_bkey_.alloc(2 * (size_t)std::max(nq, 1)));
    if (nu > 0) EDLIB_AMD_HIP(hipMemcpy(d_uq_.p, unitQuery, (size_t)nu * sizeof(int), hipMemcpyHostToDevice));

    // ---- the window kernel's share
    std::vector<std::vector<int>> byWords(kCrossMaxQueryWords + 1);       // units per word group
    size_t kernelUnits = 0;
    for (int u = 0; u < nu; ++u) {
        if (!onKernel(u)) { pairUnits_.push_back(u); continue; }
        byWords[std::max(1, (qlen(unitQuery[u]) + 31) / 32)].push_back(u);      // empty queries ride in the one-word group
        ++kernelUnits;
    }
    if (kernelUnits > 0) {
        if (uploadQueries(queries, qoff, stranded)) return 1;
        // a pool entry's slot in its group; the entry of a unit is its query, or 2 * query + strand in a stranded batch
        std::vector<int> slotOf((size_t)nq * (stranded ? 2 : 1), -1);
        for (int w = 1; w <= kCrossMaxQueryWords; ++w) {
            auto& us = byWords[w];
            if (us.empty()) continue;
            // neighbours in window length share a wave, so that its 64 lanes finish together
            std::stable_sort(us.begin(), us.end(), [&](int a, int b) { return unitLength[a] < unitLength[b]; });
            groupOf_[w].reset(new Group);
            Group* g = groupOf_[w].get();
            g->words = w; g->numSorted = (int)us.size();
            std::vector<int> perm, uslot(us.size()), ustart(us.size()), ulen(us.size());
            for (size_t i = 0; i < us.size(); ++i) {
                const int u = us[i], q = unitQuery[u], m = qlen(q), n = unitLength[u];
                const int e = stranded ? 2 * q + strandOf(u) : q;
                if (slotOf[e] < 0) { slotOf[e] = (int)perm.size(); perm.push_back(e); }    // entries that a unit names
                uslot[i] = slotOf[e]; ustart[i] = unitStart[u]; ulen[i] = n;
                if (m > 0 && n > 0 && !cross_nw_outside((int)cfg.mode, cfg.k, m, n)) g->wordSteps += (long long)w * n;
            }
            const size_t ns = us.size();
            if (allocGroup(*g, perm)) return 1;
            EDLIB_AMD_HIP(g->d_uslot.alloc(ns)); EDLIB_AMD_HIP(g->d_ustart.alloc(ns));
            EDLIB_AMD_HIP(g->d_ulen.alloc(ns)); EDLIB_AMD_HIP(g->d_uperm.alloc(ns));
            EDLIB_AMD_HIP(hipMemcpy(g->d_uslot.p, uslot.data(), ns * sizeof(int), hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(g->d_ustart.p, ustart.data(), ns * sizeof(int), hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(g->d_ulen.p, ulen.data(), ns * sizeof(int), hipMemcpyHostToDevice));
            EDLIB_AMD_HIP(hipMemcpy(g->d_uperm.p, us.data(), ns * sizeof(int), hipMemcpyHostToDevice));
            groups_.push_back(g);
        }
    }

    // ---- the pair engine's share: these units' bytes are replicated, query and window
    if (!pairUnits_.empty()) {
        PairPool pool;
        for (long long u : pairUnits_) {
            const int q = unitQuery[u];
            pool.add(queries + qoff[q], qlen(q), strandOf((int)u) != 0, target + unitStart[u], unitLength[u]);
        }
        const int np = (int)pairUnits_.size();
        pairs_.reset(new Batch);
        if (pool.init(*pairs_, cfg_, device)) return 1;
        EDLIB_AMD_HIP(h_vals_.alloc(3 * (size_t)np * sizeof(int)));
        EDLIB_AMD_HIP(d_cells_.alloc((size_t)np)); EDLIB_AMD_HIP(d_vals_.alloc(3 * (size_t)np));
        EDLIB_AMD_HIP(hipMemcpy(d_cells_.p, pairUnits_.data(), (size_t)np * sizeof(long long), hipMemcpyHostToDevice));
    }
    return 0;
}

// The queries and the units of a checked list inside the kernel's envelope made the batch's.  The raw pool, the caller's
// offsets and the unit arrays go up as they are, one asynchronous copy each; the device makes the rest
// (window_units.hip): the pool's offsets (and both strands where c.stranded), the units by (word group, window length,
// unit), a Peq slot per named entry.  The host has the units of every group from its census and reads the groups' slot
// counts back, nine ints; a group's arrays are views into the prepared ones.  What the batch held as internal pair
// session is dropped; the stream is idle afterwards.
int WindowBatch::prepareUnits(const char* queries, const long long* qoff, int nq, const int* unitQuery, const int* unitStart,
                              const int* unitLength, const unsigned char* unitStrand, int nu, const UnitCensus& c)
{
    const bool st = c.stranded;
    const size_t ne = (size_t)nq * (st ? 2 : 1), n = (size_t)nu;
    const long long qb = nq > 0 ? qoff[0] : 0, qbytes = nq > 0 ? qoff[nq] - qb : 0;
    pairs_.reset(); pairUnits_.clear();
    d_cells_.release(); d_vals_.release(); h_vals_.release();
    groups_.clear();
    nq_ = nq; nu_ = nu;
    haveRun_ = false;
    stats = EdlibAmdBatchStats{};
    stats.cells = c.cells;
    // (what a pair batch plans a gathered set from: gatherSource)
    onDevice_ = true; stranded_ = st;
    if (nq > 0) h_qoff_.assign(qoff, qoff + nq + 1); else h_qoff_.assign(1, 0);
    EDLIB_AMD_HIP(d_units_.ensure(3 * (size_t)std::max(nu, 1))); EDLIB_AMD_HIP(d_uq_.ensure((size_t)std::max(nu, 1)));
    EDLIB_AMD_HIP(d_best_.ensure(3 * (size_t)std::max(nq, 1))); EDLIB_AMD_HIP(d_bkey_.ensure(2 * (size_t)std::max(nq, 1)));

    // ---- the query pool
    EDLIB_AMD_HIP(d_qoff_.ensure(ne + 1)); EDLIB_AMD_HIP(d_qpool_.ensure((st ? 2 : 1) * (size_t)qbytes + 16));
    if (nq > 0) {
        EDLIB_AMD_HIP(prep_.offIn.ensure((size_t)nq + 1));
        EDLIB_AMD_HIP(hipMemcpyAsync(prep_.offIn.p, qoff, ((size_t)nq + 1) * sizeof(long long), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(launch_window_query_offsets(prep_.offIn.p, nq, st, d_qoff_.p, stream_));
        uint8_t* raw = d_qpool_.p;
        if (st) { EDLIB_AMD_HIP(prep_.raw.ensure((size_t)qbytes + 16)); raw = prep_.raw.p; }
        if (qbytes) EDLIB_AMD_HIP(hipMemcpyAsync(raw, queries + qb, (size_t)qbytes, hipMemcpyHostToDevice, stream_));
        if (st) EDLIB_AMD_HIP(launch_strand_pool(raw, d_qoff_.p, nq, d_qpool_.p, stream_));
    }

    // ---- the units
    if (!prep_.h_bound.p) EDLIB_AMD_HIP(prep_.h_bound.alloc((kWindowNoGroup + 1) * sizeof(int)));
    int* bound = reinterpret_cast<int*>(prep_.h_bound.p);
    memset(bound, 0, (kWindowNoGroup + 1) * sizeof(int));
    if (nu > 0) {
        UnitPrep& p = prep_;
        size_t tmpBytes = 0;
        EDLIB_AMD_HIP(window_units_tmp_bytes(nu, (int)ne, &tmpBytes));
        EDLIB_AMD_HIP(p.ustart.ensure(n)); EDLIB_AMD_HIP(p.ulen.ensure(n)); EDLIB_AMD_HIP(p.tmp.ensure(tmpBytes));
        EDLIB_AMD_HIP(p.ukey.ensure(n)); EDLIB_AMD_HIP(p.uval.ensure(n)); EDLIB_AMD_HIP(p.ukeyS.ensure(n));
        EDLIB_AMD_HIP(p.named.ensure(ne)); EDLIB_AMD_HIP(p.ekey.ensure(ne)); EDLIB_AMD_HIP(p.eval.ensure(ne));
        EDLIB_AMD_HIP(p.ekeyS.ensure(ne)); EDLIB_AMD_HIP(p.slotOf.ensure(ne)); EDLIB_AMD_HIP(p.ent.ensure(ne));
        EDLIB_AMD_HIP(p.bound.ensure(kWindowNoGroup + 1));
        EDLIB_AMD_HIP(p.suslot.ensure(n)); EDLIB_AMD_HIP(p.sustart.ensure(n)); EDLIB_AMD_HIP(p.sulen.ensure(n));
        EDLIB_AMD_HIP(p.superm.ensure(n));
        if (st) EDLIB_AMD_HIP(p.strand.ensure(n));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_uq_.p, unitQuery, n * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(p.ustart.p, unitStart, n * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(p.ulen.p, unitLength, n * sizeof(int), hipMemcpyHostToDevice, stream_));
        if (st) EDLIB_AMD_HIP(hipMemcpyAsync(p.strand.p, unitStrand, n, hipMemcpyHostToDevice, stream_));
        WindowUnitsArgs a{};
        a.offIn = p.offIn.p; a.unitQuery = d_uq_.p; a.unitStart = p.ustart.p; a.unitLength = p.ulen.p;
        a.unitStrand = st ? p.strand.p : nullptr;
        a.numUnits = nu; a.numEntries = (int)ne;
        a.named = p.named.p; a.ukey = p.ukey.p; a.uval = p.uval.p; a.ukeySorted = p.ukeyS.p;
        a.ekey = p.ekey.p; a.eval = p.eval.p; a.ekeySorted = p.ekeyS.p; a.slotOf = p.slotOf.p;
        a.entSorted = p.ent.p; a.bound = p.bound.p;
        a.uslot = p.suslot.p; a.ustart = p.sustart.p; a.ulen = p.sulen.p; a.uperm = p.superm.p;
        EDLIB_AMD_HIP(launch_window_units_prepare(a, p.tmp.p, tmpBytes, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(bound, p.bound.p, (kWindowNoGroup + 1) * sizeof(int), hipMemcpyDeviceToHost, stream_));
    }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));

    // ---- the groups that have units: views into the prepared arrays, Peq buffers of their own
    size_t at = 0;
    for (int w = 1; w <= kCrossMaxQueryWords; ++w) {
        if (c.units[w] == 0) continue;
        if (!groupOf_[w]) groupOf_[w].reset(new Group);
        Group& g = *groupOf_[w];
        const size_t ns = (size_t)c.units[w];
        g.words = w; g.numSorted = c.units[w]; g.wordSteps = c.wordSteps[w];
        g.slots = bound[w] - bound[w - 1];
        if (g.slots <= 0 || bound[w - 1] < 0 || (size_t)bound[w] > ne) {
            set_error("window batch: the device counted %d query slots for the %d units of %d words", g.slots, c.units[w], w);
            return 1;
        }
        g.d_perm.alias(prep_.ent.p + bound[w - 1], (size_t)g.slots);
        g.d_uslot.alias(prep_.suslot.p + at, ns); g.d_ustart.alias(prep_.sustart.p + at, ns);
        g.d_ulen.alias(prep_.sulen.p + at, ns); g.d_uperm.alias(prep_.superm.p + at, ns);
        const size_t blocks = (size_t)(g.slots + 63) / 64;
        EDLIB_AMD_HIP(g.d_qlen.ensure(g.slots)); EDLIB_AMD_HIP(g.d_kinit.ensure(g.slots)); EDLIB_AMD_HIP(g.d_alpha.ensure(g.slots));
        EDLIB_AMD_HIP(g.d_peq.ensure(blocks * syms_ * g.words * 64));
        groups_.push_back(&g);
        at += ns;
    }
    return 0;
}

int WindowBatch::setUnits(const char* queries, const long long* qoff, int nq, const int* unitQuery, const int* unitStart,
                          const int* unitLength, const unsigned char* unitStrand, int nu)
{
    static const char* const fn = "edlibAmdBatchWindowsSetUnits";
    // ---- what is refused leaves the batch as it was
    if (nu < 0) { set_error("%s: numUnits must be >= 0 (got %d)", fn, nu); return 1; }
    if (nq < 0) { set_error("%s: numQueries must be >= 0 (got %d)", fn, nq); return 1; }
    if (nq > 0 && (!queries || !qoff)) { set_error("%s: queries and queryOffsets must not be NULL for %d queries", fn, nq); return 1; }
    if (nu > 0 && (!unitQuery || !unitStart || !unitLength)) {
        set_error("%s: unitQuery, unitStart and unitLength must not be NULL for %d units", fn, nu);
        return 1;
    }
    if (tab_.sigmaT > kCrossMaxSyms) {
        set_error("%s: the batch's target holds %d distinct symbols, the limit for a batch that streams units is %d: create a "
                  "new batch", fn, tab_.sigmaT, kCrossMaxSyms);
        return 1;
    }
    // the host's share, linear in numQueries + numUnits: one pass over the offsets, one over the units
    for (int q = 0; q < nq; ++q) {
        const long long m = qoff[q + 1] - qoff[q];
        if (m < 0) { set_error("%s: bad query offsets (query %d ends before it starts)", fn, q); return 1; }
        if (m > 32 * kCrossMaxQueryWords) {
            set_error("%s: query %d has %s bases, the limit for a streamed set is %d: create a new batch", fn, q,
                      with_commas(m).c_str(), 32 * kCrossMaxQueryWords);
            return 1;
        }
    }
    UnitCensus census;
    if (checkUnits(qoff, nq, targetLength_, unitQuery, unitStart, unitLength, unitStrand, nu, (int)cfg_.mode, cfg_.k, census))
        return 1;
    if (census.longUnit >= 0) {
        set_error("%s: unit %d has a window of %s columns, the limit for a streamed set is %s: create a new batch", fn,
                  census.longUnit, with_commas(unitLength[census.longUnit]).c_str(), with_commas(kCrossMaxTarget).c_str());
        return 1;
    }
    if (census.stranded && nq > 0x3fffffff) { set_error("%s: bad batch shape", fn); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);

    // ---- from here a device error leaves the batch without units
    noUnits_ = true;
    if (prepareUnits(queries, qoff, nq, unitQuery, unitStart, unitLength, unitStrand, nu, census)) return 1;
    noUnits_ = false;
    return 0;
}

int WindowBatch::gatherSource(const char* fn, WindowSource& out) const
{
    if (tab_.sigmaT > kCrossMaxSyms) {
        set_error("%s: the window batch's target holds %d distinct symbols, the limit for a batch to gather pairs from is %d "
                  "(its target is not resident as a 4-bit pack): materialise the pairs and use edlibAmdBatchPairsSetPairs", fn,
                  tab_.sigmaT, kCrossMaxSyms);
        return 1;
    }
    if (noUnits_) {
        set_error("%s: the window batch has no units (edlibAmdBatchWindowsSetUnits failed on the device): set them again", fn);
        return 1;
    }
    if (!onDevice_) {
        set_error("%s: the window batch was created over a unit outside the window kernel's envelope (a query above %d bases "
                  "or a window above %s columns) and took the host route: its queries are not resident to gather from; give "
                  "it a set with edlibAmdBatchWindowsSetUnits, or materialise the pairs and use edlibAmdBatchPairsSetPairs", fn,
                  32 * kCrossMaxQueryWords, with_commas(kCrossMaxTarget).c_str());
        return 1;
    }
    out = WindowSource{};
    out.numQueries = nq_; out.targetLength = targetLength_;
    out.h_qoff = h_qoff_.data();
    out.d_qpool = d_qpool_.p; out.qpoolBytes = d_qpool_.n; out.d_qoff = d_qoff_.p; out.stranded = stranded_;
    out.d_pack = d_tpk_.p; out.packDwords = ((long long)targetLength_ + 7) / 8;
    memcpy(out.idToByte, tab_.idToByte, 16);
    return 0;
}

int WindowBatch::noResults()
{
    if (noUnits_) set_error("window batch: it has no units (edlibAmdBatchWindowsSetUnits failed on the device): set them again");
    else set_error("window batch: no results (Run it first)");
    return 1;
}

int WindowBatch::run()
{
    if (noUnits_) return noResults();
    pool_quarantine(false);
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard guard(device_);
    if (beginRun(guard.status, {&units_, &best_})) return 1;
    const size_t nu = (size_t)nu_;
    int* ed = d_units_.p; int* nloc = ed + nu; int* end = ed + 2 * nu;

    // the window kernel: Peq of every query a unit names, then one scan per word group
    const auto scanGroups = [&]() -> int {
        for (auto& g : groups_) {
            WindowScanArgs a{};
            a.peq = g->d_peq.p; a.qlen = g->d_qlen.p; a.tpk = d_tpk_.p; a.targetLength = targetLength_;
            a.uslot = g->d_uslot.p; a.ustart = g->d_ustart.p; a.ulen = g->d_ulen.p; a.uperm = g->d_uperm.p;
            a.numSorted = g->numSorted; a.kcfg = cfg_.k;
            a.ed = ed; a.nloc = nloc; a.end = end;
            EDLIB_AMD_HIP(launch_scan_windows(g->words, syms_, (int)cfg_.mode, a, stream_));
            ++stats.scan_launches;
            stats.word_steps += g->wordSteps;
        }
        return 0;
    };
    if (scanRun(groups_, 16, scanGroups)) return 1;
    // the pair engine runs on its own streams meanwhile
    if (pairs_) {
        int* vals = reinterpret_cast<int*>(h_vals_.p);
        const size_t np = pairUnits_.size();
        if (pairs_->run()) return 1;
        if (readCells(*pairs_, np, vals, "window")) return 1;
        addSessionStats(*pairs_, true);
        stats.path |= 2;
        EDLIB_AMD_HIP(hipMemcpyAsync(d_vals_.p, vals, 3 * np * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(launch_cross_scatter(d_cells_.p, d_vals_.p, (long long)np, ed, nloc, end, stream_));
    }
    EDLIB_AMD_HIP(launch_window_best(d_uq_.p, ed, nu_, nq_, d_bkey_.p, d_best_.p, stream_));
    return endRun(t0, !groups_.empty());
}

int WindowBatch::view(int what, EdlibAmdWindowView* out)
{
    if (!haveRun_) return noResults();
    if (what & ~(EDLIB_AMD_WINDOW_UNITS | EDLIB_AMD_WINDOW_BEST)) { set_error("window view: unknown parts %d", what); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const size_t unitBytes = 3 * (size_t)nu_ * sizeof(int), bestBytes = 3 * (size_t)nq_ * sizeof(int);
    if (fetchParts({{what & EDLIB_AMD_WINDOW_UNITS, &units_, d_units_.p, unitBytes},
                    {what & EDLIB_AMD_WINDOW_BEST, &best_, d_best_.p, bestBytes}})) return 1;
    memset(out, 0, sizeof *out);
    out->numUnits = nu_; out->numQueries = nq_;
    if (what & EDLIB_AMD_WINDOW_UNITS) {
        const int* p = reinterpret_cast<const int*>(units_.h.p);
        out->editDistance = p; out->numLocations = p + nu_; out->endLocation = p + 2 * (size_t)nu_;
    }
    if (what & EDLIB_AMD_WINDOW_BEST) {
        const int* b = reinterpret_cast<const int*>(best_.h.p);
        out->bestUnit = b; out->bestDistance = b + nq_; out->secondDistance = b + 2 * (size_t)nq_;
    }
    return 0;
}

}  // namespace edlib_amd
