// engine_windows.hip -- host side of window batches: units over one resident target, unit u = query unitQuery[u] against
// the window [unitStart[u], unitStart[u] + unitLength[u]), DISTANCE only (DESIGN.md "Window batches").  Create checks the
// unit list, packs the target to 4-bit codes once, sorts the queries into word groups (a cross batch's) and every group's
// units by window length, and uploads per unit its query slot, start, length and place in the caller's order; nothing is
// sized by bytes of windows.  A Run builds the Peq rows of every query, scans every group on the window kernel, lets the
// internal pair session of the units outside the kernel's envelope run meanwhile, scatters its results into the unit
// arrays and reduces them to the best unit per query.  Results stay in HBM until view() asks for a part of them.
// Units with a strand: where a unit names the reverse complement of its query the query pool holds both
// strands of every query, made on the device (entry 2 q + strand), and a Peq slot goes to each (query, strand) a kernel
// unit names; the scan and the best reduction do not know about strands.
#include "engine_lanes.hpp"

#include <algorithm>
#include <cstring>

namespace edlib_amd {

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
    for (int u = 0; u < nu; ++u) {
        if (unitQuery[u] < 0 || unitQuery[u] >= nq) {
            set_error("window batch: unit %d names query %d, outside [0, numQueries = %d)", u, unitQuery[u], nq);
            return 1;
        }
        if (unitStart[u] < 0) { set_error("window batch: unit %d has a negative unitStart (%d)", u, unitStart[u]); return 1; }
        if (unitLength[u] < 0) { set_error("window batch: unit %d has a negative unitLength (%d)", u, unitLength[u]); return 1; }
        if ((long long)unitStart[u] + (long long)unitLength[u] > (long long)targetLength) {
            set_error("window batch: unit %d ends past the target (unitStart %d + unitLength %d > targetLength %d)", u,
                      unitStart[u], unitLength[u], targetLength);
            return 1;
        }
        if (unitStrand && unitStrand[u] > 1) {
            set_error("window batch: unit %d has unitStrand %d (0: the query, 1: its reverse complement)", u, (int)unitStrand[u]);
            return 1;
        }
    }
    bool stranded = false;                                                // a unit names a reverse complement
    for (int u = 0; u < nu && unitStrand && !stranded; ++u) stranded = unitStrand[u] != 0;
    if (stranded && nq > 0x3fffffff) { set_error("bad batch shape"); return 1; }
    auto strandOf = [&](int u) { return stranded ? (int)unitStrand[u] : 0; };
    if (check_device(device)) return 1;

    keep_config(cfg, cfg_, eqs_);
    device_ = device; nq_ = nq; nu_ = nu; targetLength_ = targetLength;
    auto qlen = [&](int q) { return (int)(qoff[q + 1] - qoff[q]); };
    stats = EdlibAmdBatchStats{};
    for (int u = 0; u < nu; ++u) stats.cells += (long long)qlen(unitQuery[u]) * unitLength[u];

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
        // the target: 4-bit codes from dword 0
        if (packHostTargets(target, {0, targetLength}, {0}, {targetLength})) return 1;
        if (uploadQueries(queries, qoff, stranded)) return 1;
        // a pool entry's slot in its group; the entry of a unit is its query, or 2 * query + strand in a stranded batch
        std::vector<int> slotOf((size_t)nq * (stranded ? 2 : 1), -1);
        for (int w = 1; w <= kCrossMaxQueryWords; ++w) {
            auto& us = byWords[w];
            if (us.empty()) continue;
            // neighbours in window length share a wave, so that its 64 lanes finish together
            std::stable_sort(us.begin(), us.end(), [&](int a, int b) { return unitLength[a] < unitLength[b]; });
            std::unique_ptr<Group> g(new Group);
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
            groups_.push_back(std::move(g));
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

int WindowBatch::run()
{
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
    if (!haveRun_) { set_error("window batch: no results (Run it first)"); return 1; }
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
