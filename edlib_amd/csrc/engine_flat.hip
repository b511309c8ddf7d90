// engine_flat.hip -- flat pair batches: short independent pairs whose descriptors, scans, start locations, paths AND
// caller-facing result arrays all stay on the device (host side of the engine; see engine.hip for the general path).
//
// The reference's per-call phases (edlib.cpp:146-301: distance and end locations, :228-272 start locations, :276-289 the
// path of the first location) for a batch whose units are pairs of at most 16 blocks: nothing about such a batch needs a
// per-unit decision on the host, so a run is a fixed sequence of launches over resident descriptors, and collection is
// three small kernels + one block copied to pinned host memory (flat_results.hip).
#include "engine.hpp"
#include "flat_results.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace edlib_amd {

// flat pair path: how many units have more end locations than their list keeps (they need the exact second pass)
__global__ void __launch_bounds__(256)
count_over_kernel(const int* __restrict__ count, int n, int cap, int* __restrict__ counter)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && count[i] > cap) atomicAdd(counter, 1);
}

// flat pair path, NW with the column store: units whose band level failed (score above the level's threshold while a
// larger one was still allowed)
__global__ void __launch_bounds__(256)
count_failed_levels_kernel(const PairDesc* __restrict__ descs, const int* __restrict__ score, int n, int kcap, int* __restrict__ counter)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PairDesc d = descs[i];
    const int whole = d.qlen > d.tlen ? d.qlen : d.tlen;
    if (score[i] > d.kinit && d.kinit < whole && d.kinit < kcap) atomicAdd(counter, 1);
}

// flat pair path, HW start locations (reference edlib.cpp:228-266): every end location e of every unit gets a reverse
// prefix scan -- reversed query against the reversed prefix target[0..e], threshold = the distance, at most m + distance
// columns (:253-257).  One thread per unit writes the descriptors of its (at most posCap) scans into slots it takes from
// a counter; slotOf[u * posCap + j] remembers which scan answers location j.
__global__ void __launch_bounds__(256)
flat_start_descs_kernel(const PairDesc* __restrict__ descs, const int* __restrict__ score, const int* __restrict__ count,
                        const int* __restrict__ pos, int n, int posCap, long long revPeqBase, int ring,
                        PairDesc* __restrict__ out, int* __restrict__ slotOf, int* __restrict__ counter, int cap)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const PairDesc d = descs[u];
    const int ed = score[u];
    int c = ed < 0 ? 0 : count[u];
    c = c > posCap ? posCap : c;
    for (int j = 0; j < posCap; ++j) {
        int slot = -1;
        if (j < c) {
            const int e = pos[(long long)u * posCap + j];
            slot = atomicAdd(counter, 1);
            if (slot < cap) {
                PairDesc x{};
                x.qoff = d.qoff + d.qlen - 1; x.qstep = -1; x.qlen = d.qlen;
                x.toff = d.toff + e; x.tstep = -1;
                const long long win = (long long)e + 1 < (long long)d.qlen + ed ? (long long)e + 1 : (long long)d.qlen + ed;
                x.tlen = (int)win; x.kinit = ed;
                x.peqOff = revPeqBase + d.peqOff;
                x.posCap = 0; x.posOff = 0; x.storeOff = 0; x.auxOff = 0; x.colOff = -1; x.bandT = 0; x.skip = 0; x.ring = ring;
                out[slot] = x;
            } else slot = -1;
        }
        slotOf[(long long)u * posCap + j] = slot;
    }
}
// start = e - (last position of the reverse scan)   (edlib.cpp:260)
__global__ void __launch_bounds__(256)
flat_starts_kernel(const int* __restrict__ slotOf, const int* __restrict__ pos, const int* __restrict__ lastOfScan, long long total,
                   int* __restrict__ starts)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int s = slotOf[i];
    starts[i] = s < 0 ? 0 : pos[i] - lastOfScan[s];
}
// flat pair path, TASK_PATH of SHW / HW units (edlib.cpp:276-289): NW of the query against target[start0 .. end0] of the
// FIRST location, with the column store.  A unit without a solution, or whose first location is the empty prefix (-1:
// the host writes its m inserts), gets an inactive descriptor (threshold below |T - m|).
__global__ void __launch_bounds__(256)
flat_path_descs_kernel(const PairDesc* __restrict__ descs, const int* __restrict__ score, const int* __restrict__ count,
                       const int* __restrict__ pos, const int* __restrict__ starts, int n, int posCap,
                       const long long* __restrict__ storeBase, int ring, PairDesc* __restrict__ out)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    PairDesc x = descs[u];
    const int m = x.qlen, ed = score[u];
    const int nb = (m + 63) >> 6, W = 64 * nb - m;
    const bool lead = W > 0 && ed == m;                              // position -1 comes first
    x.posCap = 0; x.posOff = 0; x.ring = ring; x.storeOff = storeBase[u]; x.colOff = -1; x.bandT = 0; x.skip = 0; x.auxOff = 0;
    if (ed < 0 || count[u] <= 0 || lead) { x.tlen = 1; x.kinit = -1; }
    else {
        const int e0 = pos[(long long)u * posCap];
        const int s0 = starts ? starts[(long long)u * posCap] : 0;
        x.toff += s0; x.tlen = e0 - s0 + 1;
        x.kinit = m > x.tlen ? m : x.tlen;                           // every block sits on the ring: the whole matrix
    }
    out[u] = x;
}

// ------------------------------------------------------------ flat pair path

// Batches of short independent pairs (the verification step of a seed-and-extend mapper: 262,144 x 150 bp in 400 bp
// windows) were host-bound: every run rebuilt 88-byte descriptors for every unit, uploaded them, downloaded 16 end
// positions per unit and walked 160-byte records five times (22..28 ns per pair with the kernels a fifth of it).  When
// every unit is a pair of at most 16 blocks and only distances are asked for, nothing about the descriptors depends on a
// run: they are built once, on the device (flat_pairs_prepare.hip), and stay resident; a run is Peq build + one ring scan
// (whole matrix on a 4- or 16-lane ring: exact for any distance, no levels) + a census of overflowing end-location lists,
// and the results stay in HBM until results() asks for them -- the lazy form the reads path has had since round 1.
FlatShape Batch::flatShape() const
{
    FlatShape s{};
    s.scanMode = flat_.scanMode; s.k = cfg_.k; s.ring = flat_.ring; s.g32 = flatG32_;
    s.nwStore = flat_.nwStore ? 1 : 0; s.ring32 = flat_.ring32 ? 1 : 0;
    return s;
}

// One pass over the two offset arrays (n + 1 entries each, any base; sharedTarget: toff has two entries, every unit's target
// is [toff[0], toff[1]) -- a shared-target batch whose units are all pair units): are they offsets, does every pair lie
// inside the flat envelope, and the reductions the layout needs.  It stops at the first pair that fails (plan.why,
// plan.who).  qout / tout (may be null): the rebased copies.
void Batch::planFlat(const long long* qoff, const long long* toff, int n, bool sharedTarget, FlatPlan& p,
                     std::vector<long long>* qout, std::vector<long long>* tout) const
{
    const int scanMode = flatScanMode();
    const bool paths = cfg_.task == EDLIB_TASK_PATH, nwStore = paths && scanMode == EDLIB_MODE_NW;
    const long long chunkCap = 0xE0000000LL / 8;                      // 8-byte entries a ring32 launch can address
    p = FlatPlan{};
    p.n = n;
    if (qout) { qout->assign((size_t)n + 1, 0); tout->assign((size_t)n + 1, 0); }
    if (nwStore) p.cuts.push_back(0);
    const long long q0 = n > 0 ? qoff[0] : 0, t0 = n > 0 ? toff[0] : 0;
    long long chunk32 = 0;
    for (int u = 0; u < n; ++u) {
        const long long ml = qoff[u + 1] - qoff[u], tl = sharedTarget ? toff[1] - toff[0] : toff[u + 1] - toff[u];
        if (qout) { (*qout)[u + 1] = qoff[u + 1] - q0; (*tout)[u + 1] = toff[u + 1] - t0; }
        p.who = u;
        if (ml < 0) { p.why = FlatPlan::kBadQueryOffsets; return; }
        if (tl < 0) { p.why = FlatPlan::kBadTargetOffsets; return; }
        if (ml == 0) { p.why = FlatPlan::kEmptyQuery; return; }
        if (tl == 0) { p.why = FlatPlan::kEmptyTarget; return; }
        if (ml > kFlatMaxQuery) { p.why = FlatPlan::kLongQuery; return; }
        // (long targets: the general path cuts HW targets into segments when the batch alone does not fill the chip)
        if (tl > kFlatMaxTarget) { p.why = FlatPlan::kLongTarget; return; }
        const int m = (int)ml, T = (int)tl, w = flat_window(scanMode, m, T), blocks = (m + 63) / 64;
        p.maxBlocks = std::max(p.maxBlocks, blocks); p.maxWords = std::max(p.maxWords, (m + 31) / 32);
        p.totalBlocks += blocks; p.cells += (long long)m * T; p.lens += m + T;
        if (!paths) continue;
        // paths stay flat when every unit's store fits a 4-lane ring: SHW / HW queries of at most 4 blocks (whole matrix of
        // the window), NW pairs of up to 16 blocks inside the first band level; never in the Hirschberg regime (:1188-1190)
        if (scanMode != EDLIB_MODE_NW && blocks > 4) { p.why = FlatPlan::kPathBlocks; return; }
        if (needs_hirschberg(m, w)) { p.why = FlatPlan::kHirschberg; return; }
        // (the resident column store and op slots are upper bounds per unit: a batch whose bounds add up to more than a
        // slice of the HBM keeps the general path, which sizes them per chunk)
        // (8-lane rings of words.  16-lane rings -- one DPP row rotation per carried word instead of two moves and a select,
        // 34 instructions per step against 38, twice the waves -- were measured at config 5: 0.195 against 0.180 ms of scan,
        // A/B on one box; the scan is not bound by its instruction count alone)
        const long long e32 = ring32_store_entries(flatG32_, m, w);
        p.store4 += ring_store_entries(4, m, w); p.store32 += e32; p.opBytes += m + w + 8;
        if (16 * p.store4 > (32LL << 30)) { p.why = FlatPlan::kStoreCap; return; }
        if (p.opBytes > (8LL << 30)) { p.why = FlatPlan::kOpsCap; return; }
        // NW (the phase-1 scan IS the storing scan): a batch whose store exceeds what 32-bit offsets reach runs in chunks of
        // units, each scanned and walked before the next reuses the store (160,000 x 1 kb: 6.4 GB of store as two chunks)
        if (nwStore) {
            if (chunk32 + e32 > chunkCap && chunk32 > 0) { p.cuts.push_back(u); p.chunkMax32 = std::max(p.chunkMax32, chunk32); chunk32 = 0; }
            chunk32 += e32;
        }
    }
    p.who = -1;
    p.qbytes = n > 0 ? qoff[n] - q0 : 0; p.tbytes = n > 0 ? toff[sharedTarget ? 1 : n] - t0 : 0;
    if (nwStore) { p.cuts.push_back(n); p.chunkMax32 = std::max(p.chunkMax32, chunk32); }
}

int Batch::initFlatPairs()
{
    dropFlatSet();
    if (!emptyUnits_.empty() || !groups_.empty() || !longUnits_.empty()) return 0;
    if (strands_) return 0;                                         // both strands resolve from the general path's records
    if ((int)pairUnits_.size() != n_ || n_ < 1024) return 0;       // (a handful of units: the zero-copy path of solveChunk)
    if (flatScanMode() < 0) return 0;
    FlatPlan plan;
    planFlat(qoff_.data(), toff_.data(), n_, shared_, plan, nullptr, nullptr);
    if (plan.why != FlatPlan::kOk) return 0;
    return prepareFlat(plan, false);
}

// The layout of a flat set, made on the batch's stream from the resident pools and offsets (flat_pairs_prepare.hip) and
// waited for once.  census: the tables come from the device's census of the target pool (a streamed set); otherwise they
// are init()'s.  Every buffer grows only.
int Batch::prepareFlat(const FlatPlan& p, bool census)
{
    const size_t n = (size_t)p.n;
    dropFlatSet();
    FlatSet& f = flat_;
    f.scanMode = flatScanMode();
    f.paths = cfg_.task == EDLIB_TASK_PATH;
    f.nwStore = f.paths && f.scanMode == EDLIB_MODE_NW;
    f.starts = cfg_.task != EDLIB_TASK_DISTANCE && f.scanMode == EDLIB_MODE_HW;
    f.maxBlocks = p.maxBlocks; f.maxWords = p.maxWords;
    // (the smallest ring that holds every query whole; storing scans: 4 lanes.  ring32 is decided below, with the alphabet)
    f.ring = (f.paths || p.maxBlocks <= 4) ? 4 : (p.maxBlocks <= 8 ? 8 : 16);
    f.chunkStart = p.cuts;
    if (f.chunkStart.size() < 2) { f.chunkStart.assign(1, 0); f.chunkStart.push_back(p.n); }

    EDLIB_AMD_HIP(d_flatDescs_.ensure(n));
    EDLIB_AMD_HIP(d_flatOut3_.ensure(3 * n));
    EDLIB_AMD_HIP(d_flatPos_.ensure(f.scanMode == EDLIB_MODE_NW ? 1 : n * kFlatPosCap));
    EDLIB_AMD_HIP(d_flatCensus_.ensure(2));
    if (!h_flatCensus_.p) EDLIB_AMD_HIP(h_flatCensus_.alloc(2 * sizeof(int)));
    if (f.starts) {
        EDLIB_AMD_HIP(d_flatRevDescs_.ensure(n));
        f.startCap = 2 * n + 1024;
        EDLIB_AMD_HIP(d_flatStartDescs_.ensure(f.startCap));
        EDLIB_AMD_HIP(d_flatStartOut3_.ensure(3 * f.startCap));
        EDLIB_AMD_HIP(d_flatSlotOf_.ensure(n * kFlatPosCap));
        EDLIB_AMD_HIP(d_flatStartsOut_.ensure(n * kFlatPosCap));
    }
    if (f.paths) {
        // op slots (m + window + 8 bytes per unit, filled from the back) and store ranges: upper bounds that depend on the
        // set only, laid out once
        f.opsTotal = p.opBytes;
        EDLIB_AMD_HIP(d_flatOpsOff_.ensure(n + 1)); EDLIB_AMD_HIP(d_flatStoreBase_.ensure(n));
        EDLIB_AMD_HIP(d_flatOps_.ensure((size_t)f.opsTotal)); EDLIB_AMD_HIP(d_flatOpsLen_.ensure(n));
        if (!f.nwStore) { EDLIB_AMD_HIP(d_flatPathDescs_.ensure(n)); EDLIB_AMD_HIP(d_flatPathOut3_.ensure(3 * n)); }
    }
    size_t tmpBytes = 0;
    EDLIB_AMD_HIP(flat_prepare_tmp_bytes(p.n, &tmpBytes));
    EDLIB_AMD_HIP(d_flatPrepTmp_.ensure(tmpBytes + 16));
    EDLIB_AMD_HIP(d_flatPrep_.ensure(5 * (n + 1)));
    EDLIB_AMD_HIP(d_flatCuts_.ensure(f.chunkStart.size()));
    if (!d_flatPrepOut_.p) EDLIB_AMD_HIP(d_flatPrepOut_.alloc(1));
    if (!h_flatPrepOut_.p) EDLIB_AMD_HIP(h_flatPrepOut_.alloc(sizeof(FlatPrepOut)));
    // (the cut points are a member: the copy may still be on its way when this function returns on an error)
    EDLIB_AMD_HIP(hipMemcpyAsync(d_flatCuts_.p, f.chunkStart.data(), f.chunkStart.size() * sizeof(int), hipMemcpyHostToDevice, stream_));

    FlatPrepareArgs a{};
    a.n = p.n; a.shape = flatShape(); a.paths = f.paths ? 1 : 0; a.starts = f.starts ? 1 : 0;
    a.maxWords = p.maxWords; a.store32Bytes = 8 * p.store32;
    a.tpool = census ? d_tpool_.p : nullptr; a.tbytes = p.tbytes;
    a.qoff = d_qoff_.p; a.toff = d_toff_.p; a.sharedTarget = shared_ ? 1 : 0;
    a.presence = census ? d_flatPrepOut_.p->presence : d_presence_.p;
    a.cuts = d_flatCuts_.p; a.ncuts = (int)f.chunkStart.size();
    a.sizes = d_flatPrep_.p; a.peqOff = d_flatPrep_.p + 3 * (n + 1); a.storeCum = d_flatPrep_.p + 4 * (n + 1);
    a.opsOff = d_flatOpsOff_.p; a.storeBase = d_flatStoreBase_.p;
    a.descs = d_flatDescs_.p; a.revDescs = d_flatRevDescs_.p;
    a.iota = census ? d_alphaIdx_.p : nullptr;
    a.steps = d_flatPrepOut_.p->steps;
    a.tmp = d_flatPrepTmp_.p; a.tmpBytes = tmpBytes;
    EDLIB_AMD_HIP(launch_flat_prepare(a, stream_));
    EDLIB_AMD_HIP(hipMemcpyAsync(h_flatPrepOut_.p, d_flatPrepOut_.p, sizeof(FlatPrepOut), hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));                // the call's one wait: the caller's memory is free behind it
    const FlatPrepOut& out = *reinterpret_cast<const FlatPrepOut*>(h_flatPrepOut_.p);

    if (census) {
        // the tables of the set, over the bytes the census found, in ascending order (nothing a pair batch reports depends
        // on symbol ids); they follow on the stream from a pinned block of the batch's own, into the block loadFlatSet
        // made the batch's tables views of
        uint8_t present[256]; int count = 0;
        for (int b = 0; b < 256; ++b) if ((out.presence[b >> 5] >> (b & 31)) & 1u) present[count++] = (uint8_t)b;
        build_tables(tab_, present, count, eqs_.data(), (int)eqs_.size());
        if (!h_tabs_.p) EDLIB_AMD_HIP(h_tabs_.alloc(1024));
        memcpy(h_tabs_.p, tab_.tlut, 256); memcpy(h_tabs_.p + 256, tab_.idToByte, 256); memcpy(h_tabs_.p + 512, tab_.eqtbl, 512);
        EDLIB_AMD_HIP(hipMemcpyAsync(d_tabs_.p, h_tabs_.p, 1024, hipMemcpyHostToDevice, stream_));
        syms_ = peq_syms(tab_.sigmaT);
    }
    // Storing scans and walks on rings of 32-row words (ring32_kernels.hip) whenever the set allows it (flat_uses_ring32: the
    // kernels decided the same from the same census).  SHW / HW paths: queries of at most 4 blocks = 8 words, whole on an
    // 8-lane ring.
    f.ring32 = flat_uses_ring32(f.paths, f.nwStore, 8 * p.store32, flatG32_, tab_.sigmaT, p.maxWords);
    const bool chunked32 = f.ring32 && f.nwStore;
    if (!chunked32) { f.chunkStart.assign(1, 0); f.chunkStart.push_back(p.n); }
    const long long peqWords = p.totalBlocks * tab_.sigmaT;
    // reversed-query Peq rows (same layout as the forward ones, behind them)
    f.revPeqBase = peqWords;
    EDLIB_AMD_HIP(d_peq64_.ensure((size_t)(f.starts ? 2 * peqWords : peqWords)));
    if (f.paths) {
        const long long entries = chunked32 ? p.chunkMax32 : (f.ring32 ? p.store32 : p.store4);
        EDLIB_AMD_HIP(d_store_.ensure(f.ring32 ? (size_t)(entries + 1) / 2 : (size_t)entries));      // (ring32: 8-byte entries)
        if (f.ring32) EDLIB_AMD_HIP(d_tsym_.ensure(d_tpool_.n));
    }
    // the word-steps of a run over the resident descriptors never change (phase 1 of a ring32 NW batch runs on the rings of
    // 32-row words)
    f.wordSteps = (long long)out.steps[chunked32 ? 1 : 0];
    ringStepsUsed_ = false;
    flatPairs_ = true;
    return 0;
}


// ------------------------------------------------------------ streamed pairs

static const char* const kNoFlatForm = "%s: the batch's config.mode (%d) has no flat form: create a new batch";

// edlibAmdBatchPairsSetPairs: another pair set through a resident pair batch (DESIGN.md §4b "Streamed pairs").  A streamed
// set is a flat set of any count; the host walks the two offset arrays once and reads no sequence byte, everything
// derived from the pairs is made on the device (prepareFlat).  What is refused leaves the batch as it was.
int Batch::setPairs(const char* queries, const long long* qoff, const char* targets, const long long* toff, int n)
{
    static const char* const fn = "edlibAmdBatchPairsSetPairs";
    if (n < 0) { set_error("%s: numPairs must be >= 0 (got %d)", fn, n); return 1; }
    if (n > 0 && (!queries || !qoff || !targets || !toff)) {
        set_error("%s: queries, queryOffsets, targets and targetOffsets must not be NULL for %d pairs", fn, n);
        return 1;
    }
    if (flatScanMode() < 0) { set_error(kNoFlatForm, fn, (int)cfg_.mode); return 1; }
    FlatPlan plan;
    std::vector<long long> qnew, tnew;
    planFlat(qoff, toff, n, false, plan, &qnew, &tnew);
    // the pools go up as they are, 16 zero bytes behind each
    return replaceFlatSet(fn, plan, qnew, tnew, [&]() -> int {
        if (plan.qbytes) EDLIB_AMD_HIP(hipMemcpyAsync(d_qpool_.p, queries + qoff[0], (size_t)plan.qbytes, hipMemcpyHostToDevice, stream_));
        if (plan.tbytes) EDLIB_AMD_HIP(hipMemcpyAsync(d_tpool_.p, targets + toff[0], (size_t)plan.tbytes, hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemsetAsync(d_qpool_.p + plan.qbytes, 0, 16, stream_));
        EDLIB_AMD_HIP(hipMemsetAsync(d_tpool_.p + plan.tbytes, 0, 16, stream_));
        return 0;
    }) ? 1 : 0;
}

// A streamed set takes the place of the batch's: `plan` is planFlat's over the set's offsets, qnew / tnew their rebased
// copies, `fill` puts the bytes of its (one or more) pairs into the two pools on the stream (loadFlatSet).  kSetRefused: the
// first pair outside the flat envelope is named and the batch is as it was; kSetLost: an error on the device, which leaves
// the batch without pairs.
int Batch::replaceFlatSet(const char* fn, const FlatPlan& plan, std::vector<long long>& qnew, std::vector<long long>& tnew,
                          const std::function<int()>& fill)
{
    if (plan.why != FlatPlan::kOk) {
        const size_t u = (size_t)plan.who;
        refuseFlat(fn, plan, qnew[u + 1] - qnew[u], tnew[u + 1] - tnew[u]);
        return kSetRefused;
    }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);                                     // (1: kSetRefused)
    noPairs_ = true;
    if (dropForStreamedSet(plan, qnew, tnew) || loadFlatSet(plan, fill)) return kSetLost;
    noPairs_ = false;
    return 0;
}

// the first pair outside the flat envelope (plan.who, of m x T bases) and the limit it passes
void Batch::refuseFlat(const char* fn, const FlatPlan& plan, long long m, long long T) const
{
    const int u = plan.who, mode = (int)cfg_.mode;
    const char* const modeName = mode == EDLIB_MODE_HW ? "HW" : (mode == EDLIB_MODE_SHW ? "SHW" : "NW");
    switch (plan.why) {
    case FlatPlan::kBadQueryOffsets: set_error("%s: bad query offsets (query %d ends before it starts)", fn, u); break;
    case FlatPlan::kBadTargetOffsets: set_error("%s: bad target offsets (target %d ends before it starts)", fn, u); break;
    case FlatPlan::kEmptyQuery:
        set_error("%s: pair %d has an empty query (0 bases), a streamed set takes queries of 1 to %s bases: create a new batch",
                  fn, u, with_commas(kFlatMaxQuery).c_str());
        break;
    case FlatPlan::kEmptyTarget:
        set_error("%s: pair %d has an empty target (0 bases), a streamed set takes targets of 1 to %s bases: create a new batch",
                  fn, u, with_commas(kFlatMaxTarget).c_str());
        break;
    case FlatPlan::kLongQuery:
        set_error("%s: pair %d has a query of %s bases, the limit for a streamed set is %s: create a new batch", fn, u,
                  with_commas(m).c_str(), with_commas(kFlatMaxQuery).c_str());
        break;
    case FlatPlan::kLongTarget:
        set_error("%s: pair %d has a target of %s bases, the limit for a streamed set is %s: create a new batch", fn, u,
                  with_commas(T).c_str(), with_commas(kFlatMaxTarget).c_str());
        break;
    case FlatPlan::kPathBlocks:
        set_error("%s: pair %d has a query of %s bases, the limit for a streamed set with EDLIB_TASK_PATH in mode %s is 256: "
                  "create a new batch", fn, u, with_commas(m).c_str(), modeName);
        break;
    case FlatPlan::kHirschberg:
        set_error("%s: pair %d (%s x %s bases) needs the linear-space path (its matrix reaches the 1 MiB rule), a streamed "
                  "set with EDLIB_TASK_PATH stays below it: create a new batch", fn, u, with_commas(m).c_str(), with_commas(T).c_str());
        break;
    case FlatPlan::kStoreCap:
        set_error("%s: at pair %d the column stores of the set pass 32 GB, the limit for a streamed set with EDLIB_TASK_PATH: "
                  "create a new batch", fn, u);
        break;
    default:
        set_error("%s: at pair %d the op slots of the set pass 8 GB, the limit for a streamed set with EDLIB_TASK_PATH: "
                  "create a new batch", fn, u);
        break;
    }
}

// What a resident pair batch drops before another set takes its place (the device is current): everything that caches
// something about the units, and the results of the last Run.  The rebased offsets of the new set become the batch's.
int Batch::dropForStreamedSet(const FlatPlan& plan, std::vector<long long>& qnew, std::vector<long long>& tnew)
{
    const int n = plan.n;
    // (a Run whose alphabetLength nobody collected: its kernel still reads the pools that are about to change)
    if (alphaPending_ && side_) EDLIB_AMD_HIP(hipStreamSynchronize(side_));
    alphaPending_ = false;
    // everything that caches something about the units: the general path walks it when a Run of the new set falls back
    shared_ = false;
    n_ = n;
    qoff_.swap(qnew); toff_.swap(tnew);
    emptyUnits_.clear(); readUnits_.clear(); longUnits_.clear(); groups_.clear(); pairNow_.clear();
    pairUnits_.resize((size_t)n);
    for (int u = 0; u < n; ++u) pairUnits_[u] = u;
    alphaUnits_ = pairUnits_; alphaOnHost_ = false; alphaBytes_ = plan.lens;
    pairSpecsFor_.clear(); ++pairSpecsVersion_;
    levelAllReady_ = laneReady_ = false;
    results_.clear(); work_.clear(); live_.clear(); startUnits_.clear(); startWhere_.clear();
    opsKeep_.clear(); opsOwned_.clear(); fusedOps_.clear(); knownSplits_.clear();
    haveResults_ = false; viewReady_ = false; cigar_[0].ready = cigar_[1].ready = false;
    lastRunFlat_ = false; flatDone_ = false; pairsCollected_ = readsCollected_ = true;
    view_ = EdlibAmdResultsView{}; viewAlnDev_ = nullptr; viewAlnOffDev_ = nullptr;
    stats = EdlibAmdBatchStats{};
    stats.cells = plan.cells;
    algoBase_ = -1; algoDirty_ = false;
    flatPairs_ = false;
    return 0;
}

// The device's share of a streamed set: the pools sized and the offsets on their way up; `fill`; behind the pools, the
// rest is prepareFlat.
int Batch::loadFlatSet(const FlatPlan& p, const std::function<int()>& fill)
{
    const size_t n = (size_t)p.n;
    // (pools and offsets that were views into init()'s one block become buffers of their own; the block goes)
    EDLIB_AMD_HIP(d_qpool_.resize((size_t)p.qbytes + 16)); EDLIB_AMD_HIP(d_tpool_.resize((size_t)p.tbytes + 16));
    EDLIB_AMD_HIP(d_qoff_.resize(n + 1)); EDLIB_AMD_HIP(d_toff_.resize(n + 1));
    // (the tables of a streamed set are views, too: into the block prepareFlat's census fills, and into its output)
    if (!d_tabs_.p) EDLIB_AMD_HIP(d_tabs_.alloc(1024));
    if (!d_flatPrepOut_.p) EDLIB_AMD_HIP(d_flatPrepOut_.alloc(1));
    d_tlut_.alias(d_tabs_.p, 256); d_idToByte_.alias(d_tabs_.p + 256, 256); d_eqtbl_.alias(d_tabs_.p + 512, 256);
    d_presence_.alias(d_flatPrepOut_.p->presence, 8);
    // alphabetLength is counted per unit as before: its unit list (0, 1, ...) is written with the layout
    EDLIB_AMD_HIP(d_alphaIdx_.ensure(n)); EDLIB_AMD_HIP(d_alphaOut_.ensure(n));
    if (alphaPin_.n < n * sizeof(int) || !alphaPin_.p) EDLIB_AMD_HIP(alphaPin_.alloc(n * sizeof(int)));
    EDLIB_AMD_HIP(hipMemcpyAsync(d_qoff_.p, qoff_.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, stream_));
    EDLIB_AMD_HIP(hipMemcpyAsync(d_toff_.p, toff_.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, stream_));
    if (p.n == 0) {
        // no pairs: 16 zero bytes behind each (empty) pool and nothing to lay out; Run and the views are those of a batch
        // created over zero pairs
        EDLIB_AMD_HIP(hipMemsetAsync(d_qpool_.p, 0, 16, stream_));
        EDLIB_AMD_HIP(hipMemsetAsync(d_tpool_.p, 0, 16, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        d_in_.release(); h_in_.release();
        build_tables(tab_, nullptr, 0, eqs_.data(), (int)eqs_.size());
        dropFlatSet();
        return 0;
    }
    if (fill() || prepareFlat(p, true)) return 1;
    d_in_.release(); h_in_.release();                            // (behind the wait: init()'s upload came from it)
    // algorithmic bytes of a Run whose results stay on the device (startStats): a constant of the set
    algoBase_ = p.lens + 8LL * (tab_.sigmaT + 1) * p.totalBlocks + 20LL * p.n;
    return 0;
}

// ------------------------------------------------------------ pairs from a window batch

// edlibAmdBatchPairsSetWindows (DESIGN.md §4b "Pairs from a window batch"): a streamed set whose pairs are (query, strand,
// window) tuples over a window batch `src` on the same device.  The host's pass over the tuples checks them against the
// window batch's query offsets and target length and builds the offsets of the two pools by running sums; they go
// through planFlat like any streamed set.  The pools are gathered on the device from the window batch's resident query
// pool and 4-bit pack (pairs_gather.hip); the rest is setPairs'.  What is refused leaves the batch as it was.
// edlibAmdBatchPairsSetSharedWindows ("Pairs from a read batch") is the same call over what a read batch lends
// (gatherSource below: its query pool and its raw target); `fn` is the caller's name in the messages.
int Batch::setWindows(const char* fn, const WindowSource& src, const int* pairQuery, const int* pairStart,
                      const int* pairLength, const unsigned char* pairStrand, int n)
{
    if (n < 0) { set_error("%s: numPairs must be >= 0 (got %d)", fn, n); return 1; }
    if (n > 0 && (!pairQuery || !pairStart || !pairLength)) {
        set_error("%s: pairQuery, pairStart and pairLength must not be NULL for %d pairs", fn, n);
        return 1;
    }
    if (flatScanMode() < 0) { set_error(kNoFlatForm, fn, (int)cfg_.mode); return 1; }
    std::vector<long long> qnew((size_t)n + 1, 0), tnew((size_t)n + 1, 0);
    for (int p = 0; p < n; ++p) {
        const int q = pairQuery[p], start = pairStart[p], len = pairLength[p];
        if (q < 0 || q >= src.numQueries) {
            set_error("%s: pair %d names query %d, outside [0, numQueries = %d) of %s", fn, p, q, src.numQueries, src.what);
            return 1;
        }
        if (start < 0) { set_error("%s: pair %d has a negative pairStart (%d)", fn, p, start); return 1; }
        if (len < 0) { set_error("%s: pair %d has a negative pairLength (%d)", fn, p, len); return 1; }
        if ((long long)start + (long long)len > (long long)src.targetLength) {
            set_error("%s: pair %d ends past the target (pairStart %d + pairLength %d > targetLength %d)", fn, p, start, len,
                      src.targetLength);
            return 1;
        }
        if (pairStrand && pairStrand[p] > 1) {
            set_error("%s: pair %d has pairStrand %d (0: the query, 1: its reverse complement)", fn, p, (int)pairStrand[p]);
            return 1;
        }
        qnew[(size_t)p + 1] = qnew[p] + (src.h_qoff[q + 1] - src.h_qoff[q]);
        tnew[(size_t)p + 1] = tnew[p] + len;
    }
    FlatPlan plan;
    planFlat(qnew.data(), tnew.data(), n, false, plan, nullptr, nullptr);
    // the tuples go up, the pools are gathered
    const int failed = replaceFlatSet(fn, plan, qnew, tnew, [&]() -> int {
        const size_t np = (size_t)n;
        EDLIB_AMD_HIP(d_gatherTuples_.ensure(2 * np + (np + 3) / 4));
        int* const dq = d_gatherTuples_.p; int* const ds = dq + np;
        uint8_t* const dst = reinterpret_cast<uint8_t*>(ds + np);
        EDLIB_AMD_HIP(hipMemcpyAsync(dq, pairQuery, np * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(ds, pairStart, np * sizeof(int), hipMemcpyHostToDevice, stream_));
        if (pairStrand) EDLIB_AMD_HIP(hipMemcpyAsync(dst, pairStrand, np, hipMemcpyHostToDevice, stream_));
        PairsGatherArgs a{};
        a.numPairs = n; a.qoff = d_qoff_.p; a.toff = d_toff_.p; a.qbytes = plan.qbytes; a.tbytes = plan.tbytes;
        a.pairQuery = dq; a.pairStart = ds; a.pairStrand = pairStrand ? dst : nullptr;
        a.qpool = d_qpool_.p; a.tpool = d_tpool_.p;
        // The gather reads the window batch's query pool, its offsets and the target pack from THIS batch's stream.  They
        // are written by WindowBatch::prepareUnits and, at Create, by LaneEngine::packHostTargets (synchronous copies, then
        // packTargets' kernel) only, and both wait for the window batch's stream before they succeed (a Run and a view read
        // them and wait, too): nothing is in flight on them between the window batch's calls, so no event orders the two
        // streams.  A read batch's pools are written by its init alone, and its gatherSource has waited for that upload.
        // prepareFlat's wait (loadFlatSet) ends the reads before this call returns: the source batch may change or go afterwards.
        EDLIB_AMD_HIP(launch_pairs_gather(src, a, stream_));
        return 0;
    });
    if (failed == kSetLost) (void)hipStreamSynchronize(stream_);     // nothing of this batch's reads the source batch behind the call
    return failed ? 1 : 0;
}

// What a pair batch gathers its pairs from where the source is a read batch (edlibAmdBatchPairsSetSharedWindows, `fn` in
// the messages): the query pool -- entry q, or 2 q + strand of a both-strand batch, whose mates init wrote -- and the raw
// target.  d_qpool_, d_qoff_ and d_tpool_ of a read batch are written by init alone (synchronous copies, the one
// asynchronous upload of d_in_ and, both strands, the memset and launch_strand_pool behind which init waits); a Run, a
// view and a path only read them.  init ends without a wait on that upload, and the gather runs on another batch's
// stream: the wait here orders the two.  The batch is not changed: the offsets of a both-strand batch's reads, which the
// set is planned from, are a copy made at the first call.
int Batch::gatherSource(const char* fn, WindowSource& out)
{
    if (!shared_ || pairsKind_) { set_error("%s: the pairs cannot be gathered from a pair batch", fn); return 1; }
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    const int numReads = strands_ ? n_ / 2 : n_;
    if (strands_ && gatherQoff_.size() != (size_t)numReads + 1) {
        gatherQoff_.resize((size_t)numReads + 1);
        for (int i = 0; i < numReads; ++i) gatherQoff_[i] = qoff_[2 * (size_t)i] / 2;
        gatherQoff_[numReads] = qoff_[n_] / 2;
    }
    out = WindowSource{};
    out.what = "the read batch";
    out.numQueries = numReads; out.targetLength = tlen(0);
    out.h_qoff = strands_ ? gatherQoff_.data() : qoff_.data();
    out.d_qpool = d_qpool_.p; out.qpoolBytes = d_qpool_.n; out.d_qoff = d_qoff_.p; out.stranded = strands_;
    out.d_tbytes = d_tpool_.p; out.tbytesAlloc = d_tpool_.n;
    // (the gather's dword loads: launch_pairs_gather refuses the rest)
    if (!out.d_qpool || !out.d_qoff || !out.d_tbytes || (reinterpret_cast<uintptr_t>(out.d_qpool) & 3) ||
        (reinterpret_cast<uintptr_t>(out.d_tbytes) & 3)) {
        set_error("%s: the read batch's pools are not resident at a 4-byte boundary", fn);
        return 1;
    }
    return 0;
}

// ------------------------------------------------------------ pairs from a cross batch

// edlibAmdBatchPairsSetCells (DESIGN.md §4b "Pairs from a cross batch"): a streamed set whose pairs are (query, target,
// window, strand) tuples over a cross or self batch `src` on the same device.  The host's pass checks the tuples against
// the lengths the source keeps (CrossBatch::gatherSource) and builds the offsets of the two pools; they go through
// planFlat like any streamed set.  The pools are gathered on the device from the source's query pool and its pack of
// targets (pairs_gather.hip); the rest is setPairs'.  What is refused leaves the batch as it was.
int Batch::setCells(const char* fn, const CellSource& src, const int* pairQuery, const int* pairTarget, const int* pairStart,
                    const int* pairLength, const unsigned char* pairStrand, int n)
{
    if (n < 0) { set_error("%s: numPairs must be >= 0 (got %d)", fn, n); return 1; }
    if (n > 0 && (!pairQuery || !pairTarget)) {
        set_error("%s: pairQuery and pairTarget must not be NULL for %d pairs", fn, n);
        return 1;
    }
    if ((pairStart == nullptr) != (pairLength == nullptr)) {
        set_error("%s: pairStart and pairLength must both be given or both be NULL (both NULL: every pair takes its whole "
                  "target); %s is NULL alone", fn, pairStart ? "pairLength" : "pairStart");
        return 1;
    }
    if (flatScanMode() < 0) { set_error(kNoFlatForm, fn, (int)cfg_.mode); return 1; }
    std::vector<long long> qnew((size_t)n + 1, 0), tnew((size_t)n + 1, 0);
    for (int p = 0; p < n; ++p) {
        const int q = pairQuery[p], t = pairTarget[p];
        if (q < 0 || q >= src.numQueries) {
            set_error("%s: pair %d names query %d, outside [0, %s = %d) of %s", fn, p, q,
                      src.self ? "numSequences" : "numQueries", src.numQueries, src.what);
            return 1;
        }
        if (t < 0 || t >= src.numTargets) {
            set_error("%s: pair %d names target %d, outside [0, %s = %d) of %s", fn, p, t,
                      src.self ? "numSequences" : "numTargets", src.numTargets, src.what);
            return 1;
        }
        const int tlen = src.h_tlen[t];
        const int start = pairStart ? pairStart[p] : 0, len = pairLength ? pairLength[p] : tlen;
        if (start < 0) { set_error("%s: pair %d has a negative pairStart (%d)", fn, p, start); return 1; }
        if (len < 0) { set_error("%s: pair %d has a negative pairLength (%d)", fn, p, len); return 1; }
        if ((long long)start + (long long)len > (long long)tlen) {
            set_error("%s: pair %d ends past target %d (pairStart %d + pairLength %d > its length %d)", fn, p, t, start, len, tlen);
            return 1;
        }
        if (pairStrand && pairStrand[p] > 1) {
            set_error("%s: pair %d has pairStrand %d (0: the query, 1: its reverse complement)", fn, p, (int)pairStrand[p]);
            return 1;
        }
        if (!src.h_inPack || !src.h_inPack[t]) {
            set_error("%s: pair %d names target %d (%s bases), which is not resident in the 4-bit pack of %s (a target above "
                      "%s bases, a set of more than %d distinct symbols, or a set outside the kernel's envelope, ran through "
                      "an internal session at Create): materialise those pairs and use edlibAmdBatchPairsSetPairs", fn, p, t,
                      with_commas(tlen).c_str(), src.what, with_commas(kCrossMaxTarget).c_str(), kCrossMaxSyms);
            return 1;
        }
        qnew[(size_t)p + 1] = qnew[p] + src.h_qlen[q];
        tnew[(size_t)p + 1] = tnew[p] + len;
    }
    FlatPlan plan;
    planFlat(qnew.data(), tnew.data(), n, false, plan, nullptr, nullptr);
    // the tuples go up, the bases are planned, the pools are gathered
    const int failed = replaceFlatSet(fn, plan, qnew, tnew, [&]() -> int {
        const size_t np = (size_t)n;
        EDLIB_AMD_HIP(d_gatherTuples_.ensure(2 * np + 3 * np + (np + 3) / 4));
        long long* const dbase = reinterpret_cast<long long*>(d_gatherTuples_.p);        // (first: 8-byte aligned)
        int* const dq = d_gatherTuples_.p + 2 * np; int* const dt = dq + np; int* const ds = dt + np;
        uint8_t* const dst = reinterpret_cast<uint8_t*>(ds + np);
        EDLIB_AMD_HIP(hipMemcpyAsync(dq, pairQuery, np * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(dt, pairTarget, np * sizeof(int), hipMemcpyHostToDevice, stream_));
        if (pairStart) EDLIB_AMD_HIP(hipMemcpyAsync(ds, pairStart, np * sizeof(int), hipMemcpyHostToDevice, stream_));
        if (pairStrand) EDLIB_AMD_HIP(hipMemcpyAsync(dst, pairStrand, np, hipMemcpyHostToDevice, stream_));
        CellsGatherArgs a{};
        a.pools.numPairs = n; a.pools.qoff = d_qoff_.p; a.pools.toff = d_toff_.p;
        a.pools.qbytes = plan.qbytes; a.pools.tbytes = plan.tbytes;
        a.pools.pairQuery = dq; a.pools.pairStart = pairStart ? ds : nullptr; a.pools.pairStrand = pairStrand ? dst : nullptr;
        a.pools.qpool = d_qpool_.p; a.pools.tpool = d_tpool_.p;
        a.pairTarget = dt; a.pairBase = dbase;
        // The gather reads the source's query pool, its offsets, the pack, its dword offsets and the places from THIS
        // batch's stream.  They are written by the source's Create and SetTargets and by its gatherSource (the places)
        // only, and gatherSource has waited for the source's stream: nothing is in flight on them, a Run only reads them.
        // prepareFlat's wait (loadFlatSet) ends the reads before this call returns: the source may change or go afterwards.
        EDLIB_AMD_HIP(launch_pairs_gather_cells(src, a, stream_));
        return 0;
    });
    if (failed == kSetLost) (void)hipStreamSynchronize(stream_);     // nothing of this batch's reads the source behind the call
    return failed ? 1 : 0;
}

int Batch::noResults(const char* who)
{
    if (noPairs_) set_error("pair batch: it has no pairs (edlibAmdBatchPairsSetPairs failed on the device): set them again");
    else set_error("%s before a successful run() (Run it first)", who);
    return 1;
}

// ------------------------------------------------------------ a Run of a flat set

// What every flat scan shares -- the resident pools, tables and Peq rows, the end-location lists, the targets as symbol
// ids (ring32 scans) -- for `count` descriptors whose scores, counts and last columns go to out3, out3Stride apart
PairScanArgs Batch::flatScanArgs(const PairDesc* descs, int count, int* out3, size_t out3Stride) const
{
    PairScanArgs a{};
    a.descs = descs; a.numUnits = count; a.qpool = d_qpool_.p; a.tpool = d_tpool_.p;
    a.tlut = d_tlut_.p; a.sigmaT = tab_.sigmaT; a.peq = d_peq64_.p;
    a.peqRowStride = peq_row_stride(std::max(flat_.ring, flat_.maxBlocks));
    a.peqFullStride = (int)std::min<long long>((long long)a.peqRowStride * tab_.sigmaT, 1 << 20);
    a.outScore = out3; a.outCount = out3 + out3Stride; a.outLast = out3 + 2 * out3Stride; a.posPool = d_flatPos_.p;
    a.tsym = flat_.ring32 ? d_tsym_.p : nullptr;
    return a;
}

// The storing NW scan of units [u0, u0 + count) of descs (results in out3, n_ apart) and its walk into their resident op
// slots, on rings of 32-row words or on the ring of 64-row blocks.  The store and the op bytes are addressed by what the
// descriptors and opsOff hold: they take no offset.
int Batch::flatStoreAndWalk(const PairDesc* descs, int* out3, int u0, int count)
{
    PairScanArgs a = flatScanArgs(descs + u0, count, out3 + u0, (size_t)n_);
    a.store = d_store_.p;
    scanTimerStart();
    if (flat_.ring32) EDLIB_AMD_HIP(launch_scan_pairs_ring32(flatG32_, true, a, flat_.maxWords, stream_));
    else EDLIB_AMD_HIP(launch_scan_pairs_ring(flat_.ring, EDLIB_MODE_NW, true, a, stream_));
    scanTimerStop();
    TracebackArgs tb{};
    tb.descs = descs + u0; tb.numUnits = count; tb.score = out3 + u0; tb.store = d_store_.p;
    tb.ops = d_flatOps_.p; tb.opsOff = d_flatOpsOff_.p + u0; tb.opsLen = d_flatOpsLen_.p + u0;
    if (flat_.ring32) EDLIB_AMD_HIP(launch_traceback32(tb, flatG32_, stream_));
    else EDLIB_AMD_HIP(launch_traceback(tb, stream_));
    return 0;
}

// One count made on the device: the counter zeroed, count(counter) launches the kernel that adds to it, the value on its
// way to pinned memory.  Enqueued only: it is flatCensus() behind the caller's wait for the stream.
template <class Count>
int Batch::enqueueFlatCensus(Count count)
{
    EDLIB_AMD_HIP(hipMemsetAsync(d_flatCensus_.p, 0, sizeof(int), stream_));
    count(d_flatCensus_.p);
    EDLIB_AMD_HIP(hipMemcpyAsync(h_flatCensus_.p, d_flatCensus_.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
    return 0;
}

// Peq rows, the phase-1 scan, what the mode and the task add to it (reference edlib.cpp:146-301 for a batch whose every
// phase stays on the device).  fellBack: the fixed layouts do not hold this run's answer, the general path takes it.
int Batch::runPairsFlat(bool& fellBack)
{
    fellBack = false;
    stats.path |= 2;
    stats.word_steps += flat_.wordSteps;
    EDLIB_AMD_HIP(uploadEq8());
    EDLIB_AMD_HIP(launch_build_peq_pairs(d_flatDescs_.p, n_, d_qpool_.p, d_eq8_.p, d_idToByte_.p, tab_.sigmaT, d_peq64_.p, stream_));
    // the targets as symbol ids, once per run (the refills of the ring32 scans read them)
    if (flat_.ring32) EDLIB_AMD_HIP(launch_target_symbols(d_tpool_.p, d_tlut_.p, (long long)d_tpool_.n, d_tsym_.p, stream_));
    if (flat_.nwStore) return runFlatNwPaths(fellBack);       // (the phase-1 scan IS the storing scan)
    const PairScanArgs a = flatScanArgs(d_flatDescs_.p, n_, d_flatOut3_.p, (size_t)n_);
    scanTimerStart();
    EDLIB_AMD_HIP(launch_scan_pairs_ring(flat_.ring, flat_.scanMode, false, a, stream_));
    scanTimerStop();
    if (flat_.scanMode != EDLIB_MODE_NW && runFlatOverflowPass(a)) return 1;
    if (flat_.starts && runFlatStarts(fellBack)) return 1;
    if (flat_.paths && !fellBack && runFlatPaths()) return 1;
    return 0;
}

// NW paths: one band level with the column store, walked; then, whether every unit got its answer from it.  A store beyond
// the 32-bit offsets of the ring32 kernels goes chunk by chunk, each scanned and walked before the next reuses the store
// (store offsets are relative to the chunk: flat_pairs_prepare.hip); every other set is one chunk.
int Batch::runFlatNwPaths(bool& fellBack)
{
    for (size_t c = 0; c + 1 < flat_.chunkStart.size(); ++c)
        if (flatStoreAndWalk(d_flatDescs_.p, d_flatOut3_.p, flat_.chunkStart[c], flat_.chunkStart[c + 1] - flat_.chunkStart[c])) return 1;
    if (enqueueFlatCensus([&](int* counter) {
            hipLaunchKernelGGL(count_failed_levels_kernel, dim3((n_ + 255) / 256), dim3(256), 0, stream_, d_flatDescs_.p, d_flatOut3_.p, n_,
                               cfg_.k >= 0 ? cfg_.k : 0x3fffffff, counter);
        })) return 1;
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    fellBack = flatCensus() > 0;                               // some unit needs the next level: the general path has them
    return 0;
}

// SHW / HW: the census of overflowing end-location lists and, for the (rare) units with more end locations than a list
// keeps, the exact second pass: their best score is already exact, so a scan with threshold = best and a list of the
// right size finds every location (strip kernel).  a: the arguments of the phase-1 scan.
int Batch::runFlatOverflowPass(const PairScanArgs& a)
{
    if (enqueueFlatCensus([&](int* counter) {
            hipLaunchKernelGGL(count_over_kernel, dim3((n_ + 255) / 256), dim3(256), 0, stream_, d_flatOut3_.p + n_, n_, kFlatPosCap, counter);
        })) return 1;
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    flatOvf_.clear();
    if (flatCensus() == 0) return 0;
    const size_t n = (size_t)n_;
    PinBuf sc; EDLIB_AMD_HIP(sc.alloc(2 * n * sizeof(int)));
    EDLIB_AMD_HIP(hipMemcpyAsync(sc.p, d_flatOut3_.p, 2 * n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    const int* score = reinterpret_cast<const int*>(sc.p); const int* count = score + n;
    std::vector<PairDesc> d2;
    const FlatShape shape = flatShape();
    long long peqOff = 0;                                    // (the scan of flat_pairs_prepare.hip, recomputed on the way)
    for (int u = 0; u < n_; peqOff += (long long)((qlen(u) + 63) / 64) * tab_.sigmaT, ++u)
        if (count[u] > kFlatPosCap) {
            PairDesc x = flat_desc(shape, u, qoff_[u], qlen(u), tbase(u), tlen(u), peqOff);
            x.kinit = score[u]; x.posCap = count[u]; x.posOff = flatOvf_.off.back(); x.ring = 0;
            d2.push_back(x); flatOvf_.unit.push_back(u); flatOvf_.off.push_back(flatOvf_.off.back() + count[u]);
        }
    DevBuf<PairDesc> dd; DevBuf<int> s2;
    DevBuf<int>& pool2 = d_flatOvfPool_;                     // (the lists stay on the device: the collection reads them there)
    EDLIB_AMD_HIP(dd.alloc(d2.size())); EDLIB_AMD_HIP(pool2.ensure((size_t)flatOvf_.off.back())); EDLIB_AMD_HIP(s2.alloc(3 * d2.size()));
    EDLIB_AMD_HIP(hipMemcpyAsync(dd.p, d2.data(), d2.size() * sizeof(PairDesc), hipMemcpyHostToDevice, stream_));
    PairScanArgs a2 = a;
    a2.descs = dd.p; a2.numUnits = (int)d2.size(); a2.posPool = pool2.p;
    a2.outScore = s2.p; a2.outCount = s2.p + d2.size(); a2.outLast = s2.p + 2 * d2.size();
    scanTimerStart();
    EDLIB_AMD_HIP(launch_scan_pairs(flat_.scanMode, false, a2, stream_));
    scanTimerStop();
    // which list belongs to which unit, for the device-side collection
    {
        std::vector<int> at((size_t)n_, -1);
        for (size_t j = 0; j < flatOvf_.unit.size(); ++j) at[(size_t)flatOvf_.unit[j]] = (int)j;
        EDLIB_AMD_HIP(d_flatOvfAt_.ensure((size_t)n_)); EDLIB_AMD_HIP(d_flatOvfOff_.ensure(flatOvf_.off.size()));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_flatOvfAt_.p, at.data(), (size_t)n_ * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_flatOvfOff_.p, flatOvf_.off.data(), flatOvf_.off.size() * sizeof(long long), hipMemcpyHostToDevice, stream_));
    }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    stats.overflow_units += (int)d2.size();
    for (const PairDesc& x : d2) stats.word_steps += 2LL * ((x.qlen + 63) / 64) * x.tlen;
    return 0;
}

// HW start locations (reference edlib.cpp:228-266), everything on the device: descriptors of the reverse prefix scans
// written by a kernel from the phase-1 results, one ring scan over them, the starts
int Batch::runFlatStarts(bool& fellBack)
{
    const int* score = d_flatOut3_.p; const int* count = d_flatOut3_.p + n_;
    int* const startOut3 = d_flatStartOut3_.p;
    if (enqueueFlatCensus([&](int* counter) {
            hipLaunchKernelGGL(flat_start_descs_kernel, dim3((n_ + 255) / 256), dim3(256), 0, stream_, d_flatDescs_.p, score, count, d_flatPos_.p,
                               n_, kFlatPosCap, flat_.revPeqBase, flat_.ring, d_flatStartDescs_.p, d_flatSlotOf_.p, counter, (int)flat_.startCap);
        })) return 1;
    // (the reversed queries' Peq rows do not depend on the count: built while it travels)
    EDLIB_AMD_HIP(launch_build_peq_pairs(d_flatRevDescs_.p, n_, d_qpool_.p, d_eq8_.p, d_idToByte_.p, tab_.sigmaT, d_peq64_.p, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    const int nscan = flatCensus();
    if ((size_t)nscan > flat_.startCap) { fellBack = true; return 0; }
    if (nscan > 0) {
        const PairScanArgs b = flatScanArgs(d_flatStartDescs_.p, nscan, startOut3, flat_.startCap);
        scanTimerStart();
        EDLIB_AMD_HIP(launch_scan_pairs_ring(flat_.ring, EDLIB_MODE_SHW, false, b, stream_));
        scanTimerStop();
    }
    const long long total = (long long)n_ * kFlatPosCap;
    hipLaunchKernelGGL(flat_starts_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, d_flatSlotOf_.p, d_flatPos_.p,
                       startOut3 + 2 * flat_.startCap, total, d_flatStartsOut_.p);
    EDLIB_AMD_HIP(hipGetLastError());
    return 0;
}

// TASK_PATH of SHW / HW units (reference edlib.cpp:276-289): one storing NW scan per unit over its first location's
// window + the traceback into the resident op slots
int Batch::runFlatPaths()
{
    hipLaunchKernelGGL(flat_path_descs_kernel, dim3((n_ + 255) / 256), dim3(256), 0, stream_, d_flatDescs_.p, d_flatOut3_.p, d_flatOut3_.p + n_,
                       d_flatPos_.p, flat_.scanMode == EDLIB_MODE_HW ? d_flatStartsOut_.p : nullptr, n_, kFlatPosCap, d_flatStoreBase_.p, flat_.ring, d_flatPathDescs_.p);
    return flatStoreAndWalk(d_flatPathDescs_.p, d_flatPathOut3_.p, 0, n_);
}

// ---------------------------------------------------------------- collection

// CIGAR strings of format f (0 extended, 1 standard) from dense op bytes on the device: lengths, their prefix sum, the
// strings into a buffer of `cap` characters (an upper bound: a run of one op is two characters), and the offsets on their
// way to pinned host memory -- everything enqueued on `st`, nothing waited for.
int Batch::enqueueCigars(int f, const uint8_t* aln, const long long* alnOff, size_t cap, hipStream_t st)
{
    const size_t n = (size_t)n_, nblocks = (n + 255) / 256;
    const size_t words = 3 * n + nblocks + 4;
    EDLIB_AMD_HIP(d_cigWork_.ensure(2 * words));
    long long* cigLen = d_cigWork_.p + (size_t)f * words; long long* cigRel = cigLen + n; long long* blockTot = cigRel + n;
    long long* totals = blockTot + nblocks; long long* cigOff = totals + 2;
    DevBuf<char>& chars = f ? d_cigChars2_ : d_cigChars_;
    EDLIB_AMD_HIP(chars.ensure(cap));
    CigarOut& c = cigar_[f];
    if (c.offs.n < (n + 1) * sizeof(long long)) EDLIB_AMD_HIP(c.offs.alloc((n + 1) * sizeof(long long)));
    EDLIB_AMD_HIP(launch_cigars(aln, alnOff, n_, f, cigLen, cigRel, blockTot, totals, nullptr, cigOff, 0, st));
    EDLIB_AMD_HIP(launch_cigars(aln, alnOff, n_, f, cigLen, cigRel, blockTot, totals, chars.p, cigOff, 1, st));
    EDLIB_AMD_HIP(hipMemcpyAsync(c.offs.p, cigOff, (n + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    return 0;
}
// ... and, once the offsets are on the host, exactly as many characters as they say
int Batch::fetchCigars(int f, hipStream_t st)
{
    CigarOut& c = cigar_[f];
    const long long total = reinterpret_cast<const long long*>(c.offs.p)[n_];
    DevBuf<char>& chars = f ? d_cigChars2_ : d_cigChars_;
    if (total < (long long)n_ || (size_t)total > chars.n) { set_error("CIGAR: bad total"); return 1; }
    if (c.chars.n < (size_t)total) EDLIB_AMD_HIP(c.chars.alloc((size_t)total + (size_t)total / 8));
    EDLIB_AMD_HIP(hipMemcpyAsync(c.chars.p, chars.p, (size_t)total, hipMemcpyDeviceToHost, st));
    return 0;
}

// The block of a device-made view, the same on the device and in pinned host memory (the members' order IS the layout)
// (what the host wants first -- the D2H of this head is most of what a DISTANCE batch brings over -- then the device's
// scratch; status is all zeros for such a batch and is filled in on the host)
struct ViewLayout {
    const size_t n, nblocks = (n + 255) / 256;
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at = (at + bytes + 63) & ~(size_t)63; return o; }
    const size_t oTotals = take(16);
    const size_t oEd = take(n * 4), oNloc = take(n * 4), oAlpha = take(n * 4);
    const size_t oLocOff = take((n + 1) * 8), oAlnOff = take((n + 1) * 8);
    const size_t headBytes = at;
    const size_t oStatus = take(n * 4), oAlnLen = take(n * 4), oBlockLoc = take(nblocks * 8), oBlockAln = take(nblocks * 8);
    const size_t hostHead = headBytes + ((n * 4 + 63) & ~(size_t)63);     // host: the head + the status array
    size_t oEnds = 0, oStarts = 0, oAln = 0;      // the view appends its own areas and sets these (oStarts = 0: no start locations)
    void bind(FlatResultArgs& a, uint8_t* dv) const {                      // what flat_results.hip writes, into the block at dv
        a.status = reinterpret_cast<int*>(dv + oStatus); a.editDistance = reinterpret_cast<int*>(dv + oEd);
        a.numLocations = reinterpret_cast<int*>(dv + oNloc); a.alphabetLength = reinterpret_cast<int*>(dv + oAlpha);
        a.alnLen = reinterpret_cast<int*>(dv + oAlnLen);
        a.locOff = reinterpret_cast<long long*>(dv + oLocOff); a.alnOff = reinterpret_cast<long long*>(dv + oAlnOff);
        a.blockLoc = reinterpret_cast<long long*>(dv + oBlockLoc); a.blockAln = reinterpret_cast<long long*>(dv + oBlockAln);
        a.ends = reinterpret_cast<int*>(dv + oEnds); a.starts = oStarts ? reinterpret_cast<int*>(dv + oStarts) : nullptr;
        a.aln = dv + oAln;
    }
};

// the variable part of a view in its pinned host block: the totals, and where the start locations and the op bytes begin
struct ViewVar { long long nloc = 0, naln = 0; size_t oStarts = 0, oAln = 0; };

// ---- the fixed part (per-unit fields, offsets, totals): waited for, checked, published; then the variable part's block
int Batch::fetchViewHead(const ViewLayout& L, long long capLoc, long long capAln, const char* who, ViewVar& var)
{
    uint8_t* const hv = h_view_.p;
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));        // (the caller queued the head copy, and what rides the same wait)
    const long long* totals = reinterpret_cast<const long long*>(hv + L.oTotals);
    const long long nloc = var.nloc = totals[0], naln = var.naln = totals[1];
    if (nloc < 0 || nloc > capLoc || naln < 0 || naln > capAln) { set_error("%s: totals out of range", who); return 1; }
    // the variable part in a pinned block of its own, sized by what there is (a block for everything a batch COULD have --
    // 146 MB of op slots for 262,144 x 150 bp HW paths that come to 39 MB -- cost its pinning on the first collection)
    const size_t vStarts = var.oStarts = ((size_t)nloc * 4 + 63) & ~(size_t)63, vAln = var.oAln = vStarts + (L.oStarts ? vStarts : 0);
    const size_t varBytes = vAln + (size_t)naln + 64;
    if (h_viewVar_.n < varBytes) EDLIB_AMD_HIP(h_viewVar_.alloc(varBytes + varBytes / 8));
    uint8_t* const hvar = h_viewVar_.p;
    view_ = EdlibAmdResultsView{};
    view_.numUnits = (int)L.n;
    memset(hv + L.headBytes, 0, L.n * 4);                // status: every unit of such a batch is EDLIB_STATUS_OK
    view_.status = reinterpret_cast<const int*>(hv + L.headBytes); view_.editDistance = reinterpret_cast<const int*>(hv + L.oEd);
    view_.numLocations = reinterpret_cast<const int*>(hv + L.oNloc); view_.alphabetLength = reinterpret_cast<const int*>(hv + L.oAlpha);
    view_.locOffsets = reinterpret_cast<const long long*>(hv + L.oLocOff); view_.alnOffsets = reinterpret_cast<const long long*>(hv + L.oAlnOff);
    view_.endLocations = reinterpret_cast<const int*>(hvar);
    view_.startLocations = L.oStarts ? reinterpret_cast<const int*>(hvar + vStarts) : nullptr;
    viewAlnDev_ = nullptr; viewAlnOffDev_ = nullptr;
    return 0;
}

// The caller-facing arrays of the last flat run, made on the device (flat_results.hip) and brought over as ONE block of
// pinned host memory: what edlibAmdBatchResultsView() hands out, what the per-unit records and the malloc'd arrays of the
// older entry points are copied from.  Valid until the next run().
int Batch::buildFlatView()
{
    if (viewReady_) return 0;
    const int scanMode = flat_.scanMode;
    const size_t n = (size_t)n_;
    const bool wantStarts = cfg_.task != EDLIB_TASK_DISTANCE, wantPath = flat_.paths;
    const long long capLoc = (scanMode == EDLIB_MODE_NW ? (long long)n : (long long)n * (kFlatPosCap + 1)) + flatOvf_.off.back();
    const long long capAln = wantPath ? flat_.opsTotal : 0;
    ViewLayout L{n};
    // (device: room for every location / op byte the batch could have; host: the fixed part now, the rest once the totals are known)
    L.oEnds = L.take((size_t)capLoc * 4); L.oStarts = wantStarts ? L.take((size_t)capLoc * 4) : 0; L.oAln = L.take((size_t)capAln + 16);
    EDLIB_AMD_HIP(d_view_.ensure(L.at));
    if (h_view_.n < L.hostHead) EDLIB_AMD_HIP(h_view_.alloc(L.hostHead));
    uint8_t* const dv = d_view_.p; uint8_t* const hv = h_view_.p;
    FlatResultArgs a{};
    a.descs = d_flatDescs_.p; a.n = n_; a.mode = scanMode; a.k = cfg_.k; a.wantPath = wantPath ? 1 : 0; a.posCap = kFlatPosCap;
    a.score = d_flatOut3_.p; a.count = d_flatOut3_.p + n; a.pos = d_flatPos_.p;
    a.devStarts = flat_.starts ? d_flatStartsOut_.p : nullptr;
    if (!flatOvf_.unit.empty()) { a.ovfAt = d_flatOvfAt_.p; a.ovfOff = d_flatOvfOff_.p; a.ovfPos = d_flatOvfPool_.p; }
    // alphabetLength comes from the side stream's kernel (or, for a handful of short sequences, from the host below)
    const bool alphaOnDevice = alphaPending_ && !alphaOnHost_ && alphaUnits_.size() == n;
    if (alphaOnDevice) { EDLIB_AMD_HIP(hipStreamWaitEvent(stream_, evB_.e, 0)); a.alphabet = d_alphaOut_.p; }
    if (wantPath) { a.opsLen = d_flatOpsLen_.p; a.opsOff = d_flatOpsOff_.p; a.ops = d_flatOps_.p; }
    L.bind(a, dv);
    EDLIB_AMD_HIP(launch_flat_results(a, reinterpret_cast<long long*>(dv + L.oTotals), stream_));
    // A PATH batch whose caller asked for CIGARs after an earlier run gets them made NOW, on the side stream, while the op
    // bytes travel: the run-length encoding of both formats (0.16 ms of kernels for config 5) overlaps the 10 MB copy
    // instead of following it, and shares its synchronisations.  (The first request of a session is served on demand.)
    bool prefetchCigars = cigarSticky_ && wantPath && capAln > 0;
    if (prefetchCigars) {
        if (!side_) EDLIB_AMD_HIP(pool_stream(&side_));
        EDLIB_AMD_HIP(evView_.create());
        EDLIB_AMD_HIP(hipEventRecord(evView_.e, stream_));
        EDLIB_AMD_HIP(hipStreamWaitEvent(side_, evView_.e, 0));
        // Best effort: the prefetch sizes its character buffers for the worst case (two characters per op slot, both formats)
        // before the totals are known.  When that does not fit the device the view is still good -- the strings are then made
        // on demand (cigarView), sized by what there is.
        for (int f = 0; f < 2 && prefetchCigars; ++f)
            if (enqueueCigars(f, dv + L.oAln, reinterpret_cast<const long long*>(dv + L.oAlnOff), (size_t)(2 * capAln) + n + 64, side_)) {
                prefetchCigars = false;
                (void)hipGetLastError();
                (void)hipStreamSynchronize(side_);               // (whatever of it was queued is over before its buffers are asked for again)
                d_cigChars_.release(); d_cigChars2_.release();
            }
    }
    EDLIB_AMD_HIP(hipMemcpyAsync(hv, dv, L.headBytes, hipMemcpyDeviceToHost, stream_));
    ViewVar var;
    if (fetchViewHead(L, capLoc, capAln, "flat results", var)) return 1;
    const long long nloc = var.nloc, naln = var.naln;
    const size_t vStarts = var.oStarts, vAln = var.oAln;
    uint8_t* const hvar = h_viewVar_.p;
    if (nloc) EDLIB_AMD_HIP(hipMemcpyAsync(hvar, dv + L.oEnds, (size_t)nloc * 4, hipMemcpyDeviceToHost, stream_));
    if (nloc && wantStarts) EDLIB_AMD_HIP(hipMemcpyAsync(hvar + vStarts, dv + L.oStarts, (size_t)nloc * 4, hipMemcpyDeviceToHost, stream_));
    if (naln) EDLIB_AMD_HIP(hipMemcpyAsync(hvar + vAln, dv + L.oAln, (size_t)naln, hipMemcpyDeviceToHost, stream_));
    if (prefetchCigars) {                              // the strings: as many characters as the offsets say (the side stream has them)
        EDLIB_AMD_HIP(hipStreamSynchronize(side_));
        for (int f = 0; f < 2; ++f) if (fetchCigars(f, side_)) return 1;
        EDLIB_AMD_HIP(hipStreamSynchronize(side_));
        for (int f = 0; f < 2; ++f) { cigar_[f].p = reinterpret_cast<const char*>(cigar_[f].chars.p); cigar_[f].off = reinterpret_cast<const long long*>(cigar_[f].offs.p); cigar_[f].ready = true; }
    }
    if (alphaPending_ && !alphaOnDevice) { EDLIB_AMD_HIP(hipStreamSynchronize(side_)); }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    alphaPending_ = false;
    view_.alignment = wantPath ? hvar + vAln : nullptr;
    viewAlnDev_ = dv + L.oAln; viewAlnOffDev_ = reinterpret_cast<const long long*>(dv + L.oAlnOff);
    // ---- what the device does not know
    int* alpha = reinterpret_cast<int*>(hv + L.oAlpha);
    if (!alphaOnDevice) {
        if (alphaOnHost_) {
            // a handful of short sequences: counted on the host from the staging block of init() (alphabetLengthsEnd's rule)
            std::vector<UnitResult> tmp(n);
            if (alphabetLengthsEnd(tmp)) return 1;
            for (size_t u = 0; u < n; ++u) alpha[u] = tmp[u].alphabetLength;
        } else if (alphaPin_.p && alphaUnits_.size() == n) {
            memcpy(alpha, alphaPin_.p, n * sizeof(int));
        }
    }
    // start locations beyond the 16 a unit's flat list keeps (a unit of the exact second pass, HW): their reverse scans run now
    if (flat_.starts && !flatOvf_.unit.empty()) {
        int* starts = reinterpret_cast<int*>(hvar + vStarts);
        std::vector<UnitSpec> late; std::vector<long long> where;
        for (int u : flatOvf_.unit) {
            const int ed = view_.editDistance[u], m = qlen(u);
            if (ed < 0) continue;
            const long long lo = view_.locOffsets[u]; const int cnt = view_.numLocations[u];
            const int lead = (cnt > 0 && view_.endLocations[lo] == -1) ? 1 : 0;
            for (int j = lead + kFlatPosCap; j < cnt; ++j) {
                const int e = view_.endLocations[lo + j];
                const long long win = std::min<long long>((long long)e + 1, (long long)m + ed);
                late.push_back(UnitSpec{qoff_[u] + m - 1, m, -1, tbase(u) + e, (int)win, -1, ed});
                where.push_back(lo + j);
            }
        }
        if (!late.empty()) {
            SolveOut so;
            if (solveSemiGlobal(EDLIB_MODE_SHW, false, late, so)) return 1;
            for (size_t i = 0; i < late.size(); ++i) starts[where[i]] = view_.endLocations[where[i]] - so.last[i];      // (edlib.cpp:260)
        }
    }
    viewReady_ = true;
    return 0;
}

// the per-unit records of the older entry points, from the view
int Batch::collectPairsFlat(std::vector<UnitResult>& res)
{
    if (buildFlatView()) return 1;
    const EdlibAmdResultsView& v = view_;
    const bool wantStarts = cfg_.task != EDLIB_TASK_DISTANCE;
    for (size_t u = 0; u < (size_t)n_; ++u) {
        UnitResult& r = res[u];
        r.status = v.status[u]; r.editDistance = v.editDistance[u]; r.alphabetLength = v.alphabetLength[u];
        r.hasStarts = r.hasAlignment = false;
        const int cnt = v.numLocations[u];
        const long long lo = v.locOffsets[u];
        r.hasEnds = cnt > 0;
        r.ends.clear(); r.starts.clear();
        if (cnt > 0) r.ends.append(v.endLocations + lo, (size_t)cnt);
        if (!wantStarts || r.editDistance < 0 || !r.hasEnds) continue;
        r.hasStarts = true;
        r.starts.append(v.startLocations + lo, (size_t)cnt);
        if (cfg_.task != EDLIB_TASK_PATH || !v.alignment) continue;
        r.hasAlignment = true;                                       // (:276-289: the path of the first location)
        r.opsView = v.alignment + v.alnOffsets[u]; r.opsViewLen = (int)(v.alnOffsets[u + 1] - v.alnOffsets[u]);
    }
    pairsCollected_ = true;
    return 0;
}

// ------------------------------------------------------ the view of a DISTANCE batch of reads

// out[slots[i]] = i: the overflow index of the slots the exact second pass served (flat_results.hip: ovfAt)
__global__ void __launch_bounds__(256)
scatter_index_kernel(const int* __restrict__ slots, int count, int* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[slots[i]] = i;
}

// slot -> unit order: what flat_results.hip reads per unit, gathered from one group's per-slot arrays
__global__ void __launch_bounds__(256)
gather_group_kernel(const int* __restrict__ perm, int nslots, const int* __restrict__ best, const int* __restrict__ total,
                    const int* __restrict__ qlen, const int* __restrict__ extra, const int* __restrict__ pos, int posCap,
                    int* __restrict__ uScore, int* __restrict__ uCount, int* __restrict__ uQlen, int* __restrict__ uAlpha,
                    int* __restrict__ uPos)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int u = perm[s];
    if (u < 0) return;
    uScore[u] = best[s]; uCount[u] = total[s]; uQlen[u] = qlen[s]; uAlpha[u] = extra[s];
    // (a small group's arrays are views into pinned host memory at an odd offset: no vector loads)
    for (int i = 0; i < posCap; ++i) uPos[(size_t)u * posCap + i] = pos[(size_t)s * posCap + i];
}

// A TASK_DISTANCE run over reads-path units only leaves its results in HBM (per slot of each word-count group: best score,
// number of end locations, the first 16 of them, the lists of the exact second pass).  That is what flat_results.hip lays out
// for a flat pair batch: the caller-facing arrays are made on the device and come over as one block, no per-read record is
// built (1M reads: 63 ms of records and copies before, 15 now).  One group of all units (reads of one word count: the
// north-star shape) has slot == unit and is read in place; several groups are first gathered into unit order.  results() --
// per-unit malloc'd arrays -- still builds its records.
bool Batch::readsViewOnDevice() const
{
    if (readsCollected_ || flatPairs_ || groups_.empty() || cfg_.task != EDLIB_TASK_DISTANCE) return false;
    if (!pairUnits_.empty() || !longUnits_.empty() || !emptyUnits_.empty() || readUnits_.size() != (size_t)n_) return false;
    const int mode = (int)cfg_.mode;
    if (mode != EDLIB_MODE_NW && mode != EDLIB_MODE_SHW && mode != EDLIB_MODE_HW) return false;
    if (groups_.size() == 1 && groups_[0]->zeroCopy) return false;          // (a handful of reads: their results are on the host already)
    return true;
}

int Batch::buildReadsView()
{
    if (viewReady_) return 0;
    const int mode = (int)cfg_.mode;
    // (both strands: the units of the view are the reads, each the reported one of its two slots -- n of them cross the link)
    const size_t n = (size_t)outN();
    const bool inPlace = groups_.size() == 1 && !strands_;   // slot == unit (makeGroup lists a group's units in unit order)
    size_t novf = 0; long long ovfTotal = 0;
    for (auto& gp : groups_) { novf += gp->ovfSlots.size(); ovfTotal += gp->ovfOff.empty() ? 0 : gp->ovfOff.back(); }
    const int posCap = mode == EDLIB_MODE_NW ? 0 : kFlatPosCap;
    const long long capLoc = (mode == EDLIB_MODE_NW ? (long long)n : (long long)n * (kFlatPosCap + 1)) + ovfTotal;
    ViewLayout L{n};
    const size_t oOvfAt = L.take(novf ? n * 4 : 4), oOvfOff = L.take((novf + 1) * 8), oOvfUnits = L.take((novf + 1) * 4);
    const size_t oOvfPool = L.take(inPlace ? 4 : (size_t)ovfTotal * 4 + 4);
    const size_t oUScore = L.take(inPlace ? 4 : n * 4), oUCount = L.take(inPlace ? 4 : n * 4), oUQlen = L.take(inPlace ? 4 : n * 4), oUAlpha = L.take(inPlace ? 4 : n * 4);
    const size_t oUPos = L.take(inPlace ? 4 : n * (size_t)posCap * 4 + 4);
    const size_t oUStrand = L.take(strands_ ? 2 * n : 4);
    L.oEnds = L.take((size_t)capLoc * 4); L.oAln = L.take(64);
    EDLIB_AMD_HIP(d_view_.ensure(L.at));
    if (h_view_.n < L.hostHead) EDLIB_AMD_HIP(h_view_.alloc(L.hostHead));
    uint8_t* const dv = d_view_.p;
    FlatResultArgs a{};
    a.descs = nullptr; a.sharedT = tlen(0); a.alphaBase = tab_.sigmaT;
    a.n = (int)n; a.mode = mode; a.k = cfg_.k; a.wantPath = 0; a.posCap = kFlatPosCap;
    // ---- the per-unit inputs: in place, or gathered from the groups
    std::vector<int> ovfUnits; std::vector<long long> ovfOffAll;
    if (inPlace) {
        ReadGroup& g = *groups_[0];
        a.qlens = g.d_qlen.p; a.score = g.d_best.p; a.count = g.d_total.p; a.pos = g.d_pos.p; a.alphabet = g.d_alphaExtra.p;
        a.ovfPos = g.d_ovfPool.p;
        ovfUnits = g.ovfSlots; ovfOffAll = g.ovfOff;
    } else {
        int* uScore = reinterpret_cast<int*>(dv + oUScore); int* uCount = reinterpret_cast<int*>(dv + oUCount);
        int* uQlen = reinterpret_cast<int*>(dv + oUQlen); int* uAlpha = reinterpret_cast<int*>(dv + oUAlpha);
        int* uPos = reinterpret_cast<int*>(dv + oUPos); int* pool = reinterpret_cast<int*>(dv + oOvfPool);
        ovfOffAll.push_back(0);
        long long poolAt = 0;
        for (auto& gp : groups_) {
            ReadGroup& g = *gp;
            if (strands_)
                EDLIB_AMD_HIP(launch_gather_group_strands(g.d_perm.p, g.nslots, g.d_win.p, g.d_best.p, g.d_total.p, g.d_qlen.p,
                                                          g.d_alphaExtra.p, g.d_pos.p, posCap, uScore, uCount, uQlen, uAlpha, uPos,
                                                          dv + oUStrand, dv + oUStrand + n, stream_));
            else
            hipLaunchKernelGGL(gather_group_kernel, dim3((unsigned)((g.nslots + 255) / 256)), dim3(256), 0, stream_,
                               g.d_perm.p, g.nslots, g.d_best.p, g.d_total.p, g.d_qlen.p, g.d_alphaExtra.p, g.d_pos.p, posCap,
                               uScore, uCount, uQlen, uAlpha, uPos);
            EDLIB_AMD_HIP(hipGetLastError());
            for (size_t i = 0; i < g.ovfSlots.size(); ++i) {
                ovfUnits.push_back(strands_ ? g.perm[g.ovfSlots[i]] >> 1 : g.perm[g.ovfSlots[i]]);
                ovfOffAll.push_back(poolAt + g.ovfOff[i + 1]);
            }
            const long long mine = g.ovfOff.empty() ? 0 : g.ovfOff.back();
            if (mine) EDLIB_AMD_HIP(hipMemcpyAsync(pool + poolAt, g.d_ovfPool.p, (size_t)mine * sizeof(int), hipMemcpyDeviceToDevice, stream_));
            poolAt += mine;
        }
        a.qlens = uQlen; a.score = uScore; a.count = uCount; a.pos = uPos; a.alphabet = uAlpha; a.ovfPos = pool;
    }
    if (novf) {
        // (pageable sources: the lists are a few thousand entries; the stream is synchronised below before they go out of scope)
        EDLIB_AMD_HIP(hipMemsetAsync(dv + oOvfAt, 0xff, n * 4, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(dv + oOvfUnits, ovfUnits.data(), novf * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(dv + oOvfOff, ovfOffAll.data(), (novf + 1) * sizeof(long long), hipMemcpyHostToDevice, stream_));
        hipLaunchKernelGGL(scatter_index_kernel, dim3((unsigned)((novf + 255) / 256)), dim3(256), 0, stream_,
                           reinterpret_cast<const int*>(dv + oOvfUnits), (int)novf, reinterpret_cast<int*>(dv + oOvfAt));
        EDLIB_AMD_HIP(hipGetLastError());
        a.ovfAt = reinterpret_cast<const int*>(dv + oOvfAt); a.ovfOff = reinterpret_cast<const long long*>(dv + oOvfOff);
    } else a.ovfPos = nullptr;
    L.bind(a, dv);
    EDLIB_AMD_HIP(launch_flat_results(a, reinterpret_cast<long long*>(dv + L.oTotals), stream_));
    EDLIB_AMD_HIP(hipMemcpyAsync(h_view_.p, dv, L.headBytes, hipMemcpyDeviceToHost, stream_));
    if (strands_ && n) EDLIB_AMD_HIP(hipMemcpyAsync(h_strand_.p, dv + oUStrand, 2 * n, hipMemcpyDeviceToHost, stream_));
    ViewVar var;
    if (fetchViewHead(L, capLoc, 0, "reads view", var)) return 1;
    const long long nloc = var.nloc;
    if (nloc) EDLIB_AMD_HIP(hipMemcpyAsync(h_viewVar_.p, dv + L.oEnds, (size_t)nloc * 4, hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    viewReady_ = true;
    if (getenv("EDLIB_AMD_DEBUG")) fprintf(stderr, "[edlib_amd] reads view made on the device: %d units in %zu group(s), %lld locations, %zu lists of the exact pass\n", (int)n, groups_.size(), nloc, novf);
    return 0;
}

int Batch::ensureCollected()
{
    if (readsCollected_ && pairsCollected_) return 0;
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    if (results_.size() != (size_t)n_) results_.assign((size_t)n_, UnitResult{});
    if (!readsCollected_ && collectReads(results_)) return 1;
    if (!pairsCollected_ && collectPairsFlat(results_)) return 1;
    return 0;
}


}  // namespace edlib_amd
