// engine_reads.hip -- host side of the reads-per-lane path: many short queries against one shared target.
// The reference's k-doubling loop around myersCalcEditDistanceSemiGlobal (edlib.cpp:197-217, 550-704), once per BATCH:
// Peq rows, a probe that picks the first threshold and the levels in between, the banded first pass, the full-height pass
// over what it left open, the exact second pass for end-location lists that did not fit, and the collection.
#include "engine.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

namespace edlib_amd {

// full-height pass of the reads path: a lane's threshold drops to what a scan of the target's first columns found
__global__ void __launch_bounds__(256)
seed_thresholds_kernel(int* __restrict__ kinit, const int* __restrict__ best, const int* __restrict__ cnt, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && cnt[i] > 0 && best[i] < kinit[i]) kinit[i] = best[i];
}

// ------------------------------------------------------- reads-per-lane path

// One scan launch over a group's slots (or a subset through d_slotmap), banded or not.
int Batch::scanGroup(ReadGroup& g, int mode, const int* d_slotmap, int nlanes, int kcap, const int* d_kinit,
                     int numSegments, int segLen, int warm, int* segBest, int* segCnt, int* segPos, int cap,
                     const long long* posOff, const int* posCap, bool unbanded, unsigned long long* wordSteps,
                     const uint32_t* peqDense, const int* qlenDense, int peqBottom, int* liveBest,
                     const Segment* segTable, long long tableCols)
{
    ReadScanArgs a{};
    // peqDense / qlenDense (+ d_kinit): rows rebuilt for exactly the lanes of this launch, in lane order (pass 2)
    a.peq = peqDense ? peqDense : g.d_peq.p; a.tpk = d_tpk_.p; a.trows = d_trows_.p; a.targetLength = tlen(0);
    // SHW (prefix mode: row -1 is 0, 1, 2, ...): D[m][j] >= j - m, and the best score never exceeds m (the empty prefix), so
    // no column beyond 2m can tie it -- the scan stops there instead of walking the whole shared target
    if (mode == EDLIB_MODE_SHW) a.targetLength = (int)std::min<long long>(a.targetLength, 64LL * g.nwords + 1);
    a.qlen = qlenDense ? qlenDense : g.d_qlen.p; a.kinit = d_kinit; a.slotmap = d_slotmap; a.nlanes = nlanes;
    a.numSegments = numSegments; a.segLen = segLen; a.warm = warm;
    a.segBest = segBest; a.segCnt = segCnt; a.segPos = segPos; a.cap = cap;
    a.posOff = posOff; a.posCap = posCap;
    a.kcap = kcap; a.wordSteps = wordSteps ? wordSteps : d_wordSteps_.p;
    a.filter = filterScan_ ? 1 : 0;
    a.liveBest = liveBest;
    a.segTable = segTable;                            // (scan_reads_kernel only: the other launchers refuse one)
    a.bottomAligned = peqBottom;                      // (only scan_reads_kernel reads such rows: launch_scan_reads below)
    a.chainIn = chain_.in; a.chainOut = chain_.out; a.chainSrc = chain_.src; a.chainInLanes = chain_.inLanes;
    a.chainBlocks = chain_.blocks; a.rowBase = chain_.rowBase;
    const bool chained = chain_.in != nullptr || chain_.out != nullptr;
    // full-height HW scans (pass 2 over unrelated reads): scan_reads_kernel for four symbols (register-resident rows: 288 ms
    // per 1M-read step; the full-height kernel with LDS rows picked by M0 took 314 ms there, the banded kernel at full
    // height 325 ms: measured in round 2, the variants are gone), scan_reads_full_kernel above four symbols and for the
    // long word groups
    const bool longGroup = g.nwords > kMaxReadWords;                  // no plain kernel for 12 / 16 words
    const bool fullHeight = banded_ && mode == EDLIB_MODE_HW && unbanded && (chained || syms_ > 4 || longGroup);
    const bool bandedKernel = !fullHeight && banded_ && mode == EDLIB_MODE_HW && (!unbanded || syms_ > 4 || longGroup);
    static const bool dbg = getenv("EDLIB_AMD_DEBUG") != nullptr;
    if (dbg) {
        // (the tests read this line; kernel= names the launcher taken below: tests/test_gpu_wide_rows.py)
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        fprintf(stderr, "[edlib_amd] scanGroup nwords=%d mode=%d nlanes=%d S=%d segLen=%d warm=%d cap=%d kcap=%d slotmap=%p posOff=%p rows=%s kernel=%s syms=%d\n",
                g.nwords, mode, nlanes, numSegments, segLen, warm, cap, kcap, (const void*)d_slotmap, (const void*)posOff,
                peqBottom > 1 ? "delay" : (peqBottom ? "bottom" : "top"),
                fullHeight ? "full" : (bandedKernel ? "banded" : "plain"), syms_);
        // (the line above is matched to its end by the tests: the depth of the delay rows goes on one of its own)
        if (peqBottom > 1) fprintf(stderr, "[edlib_amd] scanGroup delayRows=%d\n", peqBottom - 1);
    }
    scanTimerStart();
    // columns a lane walks: the segments' own columns (a launch may cover a prefix of the target only) and their warm-ups
    // (a table of segments comes with its own sum)
    const long long colsScanned = segTable ? tableCols
        : std::min<long long>(a.targetLength, (long long)numSegments * segLen) + (long long)(numSegments - 1) * warm;
#ifdef EDLIB_AMD_DRAIN_DIAG
    // diagnostic build (-DEDLIB_AMD_DRAIN_DIAG, never the library that ships): the clocks of every wave of the last level's
    // main launch go to edlib_amd_drain.bin in the working directory (tools/drain_model.py reads it): gridX, gridY, then the
    // entry and the exit clocks.  With -DEDLIB_AMD_DRAIN_UNIFORM as well the launch keeps the uniform plan.
    const char* drainOut = (peqBottom && liveBest) ? "edlib_amd_drain.bin" : nullptr;
    DevBuf<unsigned long long> d_clk;
    const size_t drainGX = ((size_t)(nlanes + 63) / 64 + 3) / 4, drainWaves = drainGX * numSegments * 4;
    if (drainOut) {
        EDLIB_AMD_HIP(d_clk.alloc(2 * drainWaves));
        EDLIB_AMD_HIP(hipMemsetAsync(d_clk.p, 0, 2 * drainWaves * sizeof(unsigned long long), stream_));
        a.waveClock = d_clk.p;
    }
#endif
    if (peqBottom && (fullHeight || bandedKernel)) EDLIB_AMD_HIP(hipErrorInvalidValue);   // rows only scan_reads_kernel reads
    if (fullHeight) {
        EDLIB_AMD_HIP(launch_scan_reads_full(g.nwords, syms_, a, stream_));
        stats.word_steps += (long long)((nlanes + 63) / 64 * 64) * g.nwords * colsScanned;
    } else if (bandedKernel) EDLIB_AMD_HIP(launch_scan_reads_banded(g.nwords, syms_, a, stream_));
    else {
        EDLIB_AMD_HIP(launch_scan_reads(g.nwords, mode, a, stream_));
        stats.word_steps += (long long)((nlanes + 63) / 64 * 64) * g.nwords * colsScanned;
    }
    scanTimerStop();
#ifdef EDLIB_AMD_DRAIN_DIAG
    if (drainOut) {
        std::vector<unsigned long long> clk(2 * drainWaves);
        EDLIB_AMD_HIP(hipMemcpyAsync(clk.data(), d_clk.p, clk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        if (FILE* f = fopen(drainOut, "wb")) {
            const unsigned long long head[2] = {drainGX, (unsigned long long)numSegments};
            fwrite(head, sizeof head, 1, f); fwrite(clk.data(), sizeof(unsigned long long), clk.size(), f); fclose(f);
        }
    }
#endif
    if (dbg) {
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        fprintf(stderr, "[edlib_amd] scanGroup done\n");
    }
    return 0;
}

// segmentation of a launch over `nlanes` lanes: enough waves to fill the chip, segments >= 4096 columns
void plan_segments(int nlanes, int T, int mode, int warmFull, long long wantWaves,
                          int& S, int& segLen, int& warm, int minSegCols)
{
    plan_segments_uniform(nlanes, T, mode == EDLIB_MODE_HW, warmFull, wantWaves, minSegCols, S, segLen, warm);   // segment_plan.hpp
}

int Batch::runReads()
{
    if (groups_.empty()) return 0;
    stats.path |= 1;
    bool seed = false;
    for (auto& gp : groups_) seed = seed || seedThreshold(*gp, false) >= 0;
    if (seed && buildSeedIndex()) return 1;
    for (auto& gp : groups_) if (runGroupScans(*gp, false)) return 1;
    // both strands: what every mate pair reports, before the exact pass (it serves the reported slots only)
    const int mode = (cfg_.mode == EDLIB_MODE_HW || cfg_.mode == EDLIB_MODE_SHW) ? (int)cfg_.mode : (int)EDLIB_MODE_NW;
    for (auto& gp : groups_)
        if (gp->mates) EDLIB_AMD_HIP(launch_resolve_strands(gp->d_perm.p, gp->d_best.p, gp->d_total.p, gp->nslots, mode, cfg_.k,
                                                            gp->d_win.p, stream_));
    for (auto& gp : groups_) if (runGroupExact(*gp)) return 1;
    return 0;
}

// The scans of one group: Peq rows, then the k-doubling levels (fullOnly: one pass at the full threshold on the
// full-height kernel -- units the piece filter handed back, whose band is the whole query).
int Batch::runGroupScans(ReadGroup& g, bool fullOnly)
{
    const int T = tlen(0);
    // unknown mode values are computed as NW (edlib.cpp:205-215)
    const int mode = (cfg_.mode == EDLIB_MODE_HW || cfg_.mode == EDLIB_MODE_SHW) ? (int)cfg_.mode : (int)EDLIB_MODE_NW;
    const bool banded = banded_ && mode == EDLIB_MODE_HW;
    const int kNoCap = 0x3fffffff;
    static const bool dbgLadder = getenv("EDLIB_AMD_DEBUG") != nullptr;
    EDLIB_AMD_HIP(launch_build_peq_reads(g.nwords, syms_, d_qpool_.p, d_qoff_.p, g.d_perm.p, g.nslots,
                                         d_eqtbl_.p, d_presence_.p, cfg_.k, g.d_peq.p, g.d_qlen.p,
                                         g.d_kinit.p, g.d_alphaExtra.p, stream_));
    // ---- pass 1: all slots; banded: threshold min(k, kFirst)
    // first threshold of the k-doubling (edlib.cpp:197-217 starts at 64): 8 up to 512 bases; the groups of 24 / 32
    // words take 12 / 16 -- at 1 % error a 1024-base read has distance ~10, and a read that fails the first level
    // pays the full 32-word height over the whole target
    // Groups the exact seed filter takes start at its threshold k_f instead: pass 1 costs them the lookups and
    // the windows, not a band over every column, and the probe below only prices the levels after it.
    const int kSeed = seedThreshold(g, fullOnly);
    const int kFirstMax = kSeed >= 0 ? kSeed : std::max(8, g.nwords / 2);
    int kFirst = (kSeed >= 0 && cfg_.k >= 0) ? std::min(kSeed, cfg_.k) : kFirstMax;
    bool twoPass = !fullOnly && banded && (cfg_.k < 0 || cfg_.k > kFirst) && 32 * g.nwords > kFirst;
    std::vector<int> ladder;                    // thresholds of the banded passes between the first and the full one
    g.lvValid = false;
    // best score of the slots in `map` with thresholds capped at kc (-1: nothing <= kc)
    auto probe_scan = [&](const std::vector<int>& map, int kc, std::vector<int>& bestOut) -> int {
        const int nm = (int)map.size();
        int S2, segLen2, warm2;
        plan_segments(nm, T, mode, g.warm, 16384, S2, segLen2, warm2);
        const size_t items = (size_t)nm * S2;
        DevBuf<int> d_map, d_sb, d_sc;
        EDLIB_AMD_HIP(d_map.alloc(nm)); EDLIB_AMD_HIP(d_sb.alloc(items)); EDLIB_AMD_HIP(d_sc.alloc(items));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_map.p, map.data(), nm * sizeof(int), hipMemcpyHostToDevice, stream_));
        if (scanGroup(g, mode, d_map.p, nm, kc, g.d_kinit.p, S2, segLen2, warm2,
                      d_sb.p, d_sc.p, d_sb.p /*unused*/, 0, nullptr, nullptr)) return 1;
        std::vector<int> cnts(items), bests(items);
        EDLIB_AMD_HIP(hipMemcpyAsync(cnts.data(), d_sc.p, items * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(bests.data(), d_sb.p, items * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        bestOut.assign(nm, -1);
        for (int i = 0; i < nm; ++i) {
            int b = 0x7fffffff;
            for (int sg = 0; sg < S2; ++sg)
                if (cnts[(size_t)i * S2 + sg] > 0) b = std::min(b, bests[(size_t)i * S2 + sg]);
            if (b <= kc) bestOut[i] = b;
        }
        return 0;
    };
    // ---- the levels between the first and the full threshold (the reference doubles k: edlib.cpp:197-217).  When
    // more than a tenth of the reads is still open after the first threshold, a sample of the open reads is scanned once
    // more with thresholds capped at 64: their distances say which intermediate thresholds pay.  A level at threshold t
    // costs every read that reaches it a band of about 1 + (t - 6) / 8 words per column; it pays when what it resolves
    // would otherwise meet a taller band.  All subsets of {12, 16, 24, 32, 48, 64} are priced; reads at
    // Illumina-like error rates (leftovers = unrelated sequence) keep the two levels they always had.
    // (sample: open slots to scan; nOpen of nReal: what the debug line reports)
    auto price_ladder = [&](const std::vector<int>& sample, size_t nOpen, int nReal) -> int {
        const int kTop = std::min(64, 32 * g.nwords - 1);
        std::vector<int> obest;
        if (probe_scan(sample, kTop, obest)) return 1;
        static const int cand[6] = {12, 16, 24, 32, 48, 64};
        auto words = [&](int t) { return std::min<double>(g.nwords, 1.0 + std::max(0, t - 6) / 8.0); };
        auto frac_le = [&](int t) {                           // share of the open reads with distance <= t
            size_t c = 0;
            for (int b : obest) if (b >= 0 && b <= t) ++c;
            return (double)c / (double)obest.size();
        };
        double bestCost = 1e30; int bestMask = 0;
        for (int mask = 0; mask < 64; ++mask) {
            double cost = 0.0, reach = 1.0; bool ok = true;
            for (int q = 0; q < 6; ++q) {
                if (!((mask >> q) & 1)) continue;
                if (cand[q] <= kFirst || cand[q] > kTop) { ok = false; break; }
                cost += reach * words(cand[q]);
                reach = 1.0 - frac_le(cand[q]);
            }
            if (!ok) continue;
            cost += reach * g.nwords;                         // what is left takes the full threshold
            if (cost < bestCost - 1e-9) { bestCost = cost; bestMask = mask; }
        }
        for (int q = 0; q < 6; ++q) if ((bestMask >> q) & 1) ladder.push_back(cand[q]);
        if (dbgLadder) {
            // (tests/test_gpu_seed_filter.py reads this line)
            fprintf(stderr, "[edlib_amd] ladder nwords=%d kFirst=%d open=%zu/%d levels:", g.nwords, kFirst, nOpen, nReal);
            for (int t : ladder) fprintf(stderr, " %d(%.2f)", t, frac_le(t));
            fprintf(stderr, " full\n");
        }
        return 0;
    };
    if (twoPass && g.nslots >= 16384 && kSeed < 0) {
        // k-doubling only pays when most units resolve at the small threshold (pass 1 costs ~2/NWD of a
        // full scan, unresolved units then pay the full scan on top).  Probe 2048 evenly strided slots
        // first (0.2 % of the work at 1M reads) and fall back to one full-threshold pass if fewer than
        // 30 % of them resolve (e.g. noisy long-read chemistry, unrelated sequences).
        // (2048 slots are an eighth of a 16,384-read batch: 2.5 of its 28.6 ms, and 8 MB of per-segment results to walk;
        // smaller batches probe a 32nd of their slots, at least 512)
        const int np = std::max(512, std::min(2048, g.nslots / 32));
        std::vector<int> probe(np);
        for (int i = 0; i < np; ++i) probe[i] = (int)((long long)i * g.nslots / np);
        std::vector<int> pbest;
        if (probe_scan(probe, kFirst, pbest)) return 1;
        int resolved = 0, real = 0;
        std::vector<int> hist(kFirstMax + 1, 0);                  // distances of the resolved probe reads
        std::vector<int> open;                                    // probe slots with nothing <= kFirstMax
        for (int i = 0; i < np; ++i) {
            if (g.perm[probe[i]] < 0) continue;
            ++real;
            if (pbest[i] >= 0) { ++resolved; ++hist[pbest[i]]; }
            else if (i == 0 || probe[i] != probe[i - 1]) open.push_back(probe[i]);
        }
        // The band of pass 1 is one 32-row word while the score 32 rows down stays above k + 4; against
        // unrelated sequence that score hovers around 13, so every unit of k below 8 keeps the second
        // word out more often.  Take the smallest threshold (>= 4) that still resolves 99.5 % of what 8
        // resolves: the few reads above it just join pass 2.
        if (resolved > 0) {
            int acc = 0, kq = kFirstMax;
            for (int d = 0; d <= kFirstMax; ++d) { acc += hist[d]; if (acc * 1000LL >= resolved * 995LL) { kq = d; break; } }
            kFirst = std::max(4, std::min(kFirstMax, kq));
        }
        if (real > 0 && resolved * 10 < real * 3) twoPass = false;
        if (twoPass && (int)open.size() * 10 > real && open.size() >= 32 && price_ladder(open, open.size(), real)) return 1;
    }
    std::vector<int> todo;                      // the slots of the next level, ascending
    bool haveTodo = false;
    if (kSeed >= 0) {
        // The seed pass costs little whatever resolves, and it is exact at its threshold over ALL slots: what it leaves open
        // is the probe's answer for the whole group, and the first level's slot list.
        if (runSeedPass(g, kFirst)) return 1;
        if (twoPass) {
            if (listOpenSlots(g, kFirst, todo)) return 1;
            haveTodo = true;
            if (g.nreal < 0) { g.nreal = 0; for (int u : g.perm) g.nreal += u >= 0; }
            if (g.nslots >= 16384 && todo.size() * 10 > (size_t)g.nreal && todo.size() >= 32) {
                const size_t nsm = std::min<size_t>(2048, todo.size());
                std::vector<int> sample(nsm);
                for (size_t i = 0; i < nsm; ++i) sample[i] = todo[i * todo.size() / nsm];
                if (price_ladder(sample, todo.size(), g.nreal)) return 1;
            }
        }
    } else {
        if (scanGroup(g, mode, nullptr, g.nslots, twoPass ? kFirst : kNoCap, g.d_kinit.p, g.numSegments, g.segLen,
                      g.warm, g.d_segBest.p, g.d_segCnt.p, g.d_segPos.p, 8, nullptr, nullptr, /*unbanded=*/fullOnly)) return 1;
        const bool chained = chain_.in != nullptr || chain_.out != nullptr;
        EDLIB_AMD_HIP(launch_merge_segments(g.d_segBest.p, g.d_segCnt.p, g.d_segPos.p, g.numSegments, 8,
                                            g.nslots, nullptr, 16, g.d_best.p, g.d_total.p, g.d_pos.p,
                                            g.d_flags.p, stream_, chained ? kOvfRescan : kOvfGatherGroup));
    }
    // ---- the next levels (k-doubling): slots with nothing <= the last threshold are rescanned with the next one,
    // the last time with their full threshold
    ladder.push_back(kNoCap);
    int kDone = kFirst;
    for (size_t lv = 0; twoPass && lv < ladder.size(); ++lv) {
        const int kcapL = ladder[lv];
        const bool last = kcapL == kNoCap;
        // the slots whose threshold min(k, m) is above what was tried: compacted on the device, only the list comes down
        if (!haveTodo && listOpenSlots(g, kDone, todo)) return 1;
        haveTodo = false;
        if (todo.empty()) break;
        {
            const size_t no = todo.size();
            int S2, segLen2, warm2;
            plan_segments((int)no, T, mode, g.warm, 65536, S2, segLen2, warm2);
            // The segment records of a level are the group's: they are reused from run to run (at 1M reads the positions
            // are a block the allocator's pool does not keep), and those of the last level outlive the loop -- the exact
            // pass gathers from them the lists that only overflowed the 16 positions of a slot.  The last level keeps 16
            // positions per segment instead of 8, so that a segment alone rarely overflows.
            const int capL = last ? kLastLevelCap : 8;
            // (sized below, once the launch's segments are known)
            EDLIB_AMD_HIP(g.d_lvMap.ensure(no));
            int* d_map = g.d_lvMap.p;
            EDLIB_AMD_HIP(hipMemcpyAsync(d_map, todo.data(), no * sizeof(int), hipMemcpyHostToDevice, stream_));
            // What the last level leaves over is usually unrelated sequence whose band is the whole query; there the
            // plain full-height kernel (register-resident Peq rows, no band bookkeeping) is ~12 % faster per
            // column than the banded one.  64 strided leftovers tell (one wave per segment: a quarter of the work of
            // the 256 this took before): the banded kernel reports its band
            // height (word-steps), and a band above 85 % of the words sends the pass to the plain kernel.
            bool plain = false;
            if (last && no >= 4096) {
                const int np2 = 64;
                std::vector<int> sub(np2);
                for (int i = 0; i < np2; ++i) sub[i] = todo[(size_t)((long long)i * no / np2)];
                int S3, segLen3, warm3;
                plan_segments(np2, T, mode, g.warm, 16384, S3, segLen3, warm3);
                const size_t it3 = (size_t)np2 * S3;
                DevBuf<int> d_m3, d_b3, d_c3, d_p3; DevBuf<unsigned long long> d_ws;
                EDLIB_AMD_HIP(d_m3.alloc(np2)); EDLIB_AMD_HIP(d_b3.alloc(it3)); EDLIB_AMD_HIP(d_c3.alloc(it3));
                EDLIB_AMD_HIP(d_p3.alloc(it3 * 8)); EDLIB_AMD_HIP(d_ws.alloc(1));
                EDLIB_AMD_HIP(hipMemcpyAsync(d_m3.p, sub.data(), np2 * sizeof(int), hipMemcpyHostToDevice, stream_));
                EDLIB_AMD_HIP(hipMemsetAsync(d_ws.p, 0, sizeof(unsigned long long), stream_));
                if (scanGroup(g, mode, d_m3.p, np2, kNoCap, g.d_kinit.p, S3, segLen3, warm3,
                              d_b3.p, d_c3.p, d_p3.p, 8, nullptr, nullptr, false, d_ws.p)) return 1;
                unsigned long long ws = 0;
                EDLIB_AMD_HIP(hipMemcpyAsync(&ws, d_ws.p, sizeof ws, hipMemcpyDeviceToHost, stream_));
                EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
                const double cols = (double)np2 * ((double)T + (double)(S3 - 1) * warm3);
                plain = (double)ws >= 0.85 * g.nwords * cols;
                stats.word_steps += (long long)ws;
            }
            // The leftovers are scattered over the batch: through the slot map every lane of a wave would pull its
            // rows from a different 256-byte line (16x the bytes, once per segment: 3 GB of fetch per 1M-read step
            // in round 1).  Their rows are rebuilt in lane order instead -- the builder reads each query once.
            // When the pass goes to the plain kernel (scanGroup: HW, four symbols, up to kMaxReadWords words, no chain), the
            // rebuilt rows are bottom-aligned: row m-1 at bit 31 of the last word, where the column reads the score's
            // delta with two full-rate shifts.  The pre-scan below shares them, on the same kernel.
            // Where the group's longest read leaves seven rows of its last word free, the rows carry seven delay rows above
            // row m-1 and the score moves once per eight columns; where it leaves three, three rows and once per four
            // (reads_kernels.hip: scan_reads_kernel<NWD, 2, true, R>); else bottom-aligned rows without delay rows.
            const bool bottomOk = plain && mode == EDLIB_MODE_HW && syms_ == 4 && g.nwords <= kMaxReadWords &&
                                  chain_.in == nullptr && chain_.out == nullptr;
            const int bottom = !bottomOk ? 0 : 1 + delay_rows_for(g.nwords, g.mMax);
            // The main launch over the leftovers is eight rounds of resident workgroups at 1M reads, and with uniform segments
            // its end is ragged: for the time of up to one segment every workgroup that finishes leaves its slot empty.
            // Its segments taper instead (plan_segments_tapered): the uniform length while much is left, then ever shorter
            // ones towards the target's end, so that the workgroups still running at the end are short ones.  The records
            // stay [lane][segment]; every column belongs to exactly one segment and positions are absolute, so the merge, the
            // gather of the exact pass and the reuse of these records (lvS) only see another segment count.
            std::vector<Segment> table;                              // (live until the synchronisation below)
            DevBuf<Segment> d_segTable; long long tableCols = 0;
            if (bottom && S2 > 1 && no >= 4096) {
                int resident = 0;
                EDLIB_AMD_HIP(scan_reads_resident_workgroups(g.nwords, bottom, &resident));
#ifdef EDLIB_AMD_DRAIN_UNIFORM
                resident = 0;                                        // diagnostic build: the uniform plan, as a table
#endif
                table = plan_segments_tapered(T, (int)(((no + 63) / 64 + 3) / 4), resident, warm2, segLen2);
                S2 = (int)table.size();
                for (const Segment& sg : table) tableCols += sg.cols + std::min(warm2, sg.start);
                EDLIB_AMD_HIP(d_segTable.alloc(table.size()));
                EDLIB_AMD_HIP(hipMemcpyAsync(d_segTable.p, table.data(), table.size() * sizeof(Segment), hipMemcpyHostToDevice, stream_));
            }
            const size_t items = no * (size_t)S2;
            EDLIB_AMD_HIP(g.d_lvBest.ensure(items)); EDLIB_AMD_HIP(g.d_lvCnt.ensure(items));
            EDLIB_AMD_HIP(g.d_lvPos.ensure(items * capL));
            int *d_sb = g.d_lvBest.p, *d_sc = g.d_lvCnt.p, *d_sp = g.d_lvPos.p;
            const size_t no64 = (no + 63) / 64 * 64;
            std::vector<int> perm2(no64, -1);
            for (size_t i = 0; i < no; ++i) perm2[i] = g.perm[todo[i]];
            DevBuf<int> d_perm2, d_qlen2, d_kinit2, d_extra2; DevBuf<uint32_t> d_peq2;
            EDLIB_AMD_HIP(d_perm2.alloc(no64)); EDLIB_AMD_HIP(d_qlen2.alloc(no64)); EDLIB_AMD_HIP(d_kinit2.alloc(no64));
            EDLIB_AMD_HIP(d_extra2.alloc(no64)); EDLIB_AMD_HIP(d_peq2.alloc(no64 * (size_t)syms_ * g.nwords));
            EDLIB_AMD_HIP(hipMemcpyAsync(d_perm2.p, perm2.data(), no64 * sizeof(int), hipMemcpyHostToDevice, stream_));
            EDLIB_AMD_HIP(launch_build_peq_reads(g.nwords, syms_, d_qpool_.p, d_qoff_.p, d_perm2.p, (int)no64,
                                                 d_eqtbl_.p, d_presence_.p, cfg_.k, d_peq2.p, d_qlen2.p,
                                                 d_kinit2.p, d_extra2.p, stream_, bottom));
            // Every segment starts from its lane's threshold, and a lane records a position whenever its best improves: from
            // min(k, m) an unrelated read walks down ~100 improvements per segment, each a scattered 4-byte store (1.2 GB of
            // write traffic per 1M-read step in round 2).  The first columns of the target give every lane a score that
            // some column does reach; all segments start from that one (results do not depend on it: the best over
            // the whole target is at most that score, and equal scores are still recorded).
            const int seedCols = 4096;                               // (a lone wave per SIMD: 0.27 ms)
            DevBuf<int> d_b0, d_c0, d_p0;                            // (live until the synchronisation below)
            if (mode == EDLIB_MODE_HW && last && no >= 4096 && S2 > 1 && T >= 16 * seedCols) {
                EDLIB_AMD_HIP(d_b0.alloc(no)); EDLIB_AMD_HIP(d_c0.alloc(no)); EDLIB_AMD_HIP(d_p0.alloc(no * 8));
                if (scanGroup(g, mode, nullptr, (int)no, kcapL, d_kinit2.p, 1, seedCols, 0,
                              d_b0.p, d_c0.p, d_p0.p, 8, nullptr, nullptr, plain, nullptr, d_peq2.p, d_qlen2.p, bottom)) return 1;
                hipLaunchKernelGGL(seed_thresholds_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, stream_,
                                   d_kinit2.p, d_b0.p, d_c0.p, (int)no);
                EDLIB_AMD_HIP(hipGetLastError());
            }
            // On the bottom-aligned rows the segments of a lane share one running best (ReadScanArgs::liveBest), from the
            // seeded threshold down: a segment that starts late starts from what the earlier ones found, and the out-of-line
            // hit path of the scan is entered that much less often.
            DevBuf<int> d_live2;
            if (bottom && S2 > 1) {
                EDLIB_AMD_HIP(d_live2.alloc(no64));
                EDLIB_AMD_HIP(hipMemcpyAsync(d_live2.p, d_kinit2.p, no64 * sizeof(int), hipMemcpyDeviceToDevice, stream_));
            }
            if (scanGroup(g, mode, nullptr, (int)no, kcapL, d_kinit2.p, S2, segLen2, warm2,
                          d_sb, d_sc, d_sp, capL, nullptr, nullptr, plain, nullptr, d_peq2.p, d_qlen2.p, bottom, d_live2.p,
                          d_segTable.p, tableCols)) return 1;
            EDLIB_AMD_HIP(launch_merge_segments(d_sb, d_sc, d_sp, S2, capL, (int)no, d_map, 16,
                                                g.d_best.p, g.d_total.p, g.d_pos.p, g.d_flags.p, stream_,
                                                last ? kOvfGatherLevel : kOvfRescan));
            EDLIB_AMD_HIP(hipStreamSynchronize(stream_));            // temporaries die here
            if (last) { g.lvValid = true; g.lvS = S2; g.lvCap = capL; g.lvMap.swap(todo); }
            // (tests/test_gpu_seed_filter.py reads this line)
            if (dbgLadder) fprintf(stderr, "[edlib_amd] level kcap=%d: %zu slots rescanned (plain=%d)\n", kcapL, no, (int)plain);
        }
        kDone = kcapL;
    }
    return 0;
}

// The group's slots that are still open above kDone (launch_select_open_slots), ascending, on the host.
// Both strands: a slot is open only while its mate holds no result either.  Mates are scanned at the same
// thresholds while both are open, so a mate that resolved at d <= kDone beats a slot with nothing <= kDone.
int Batch::listOpenSlots(ReadGroup& g, int kDone, std::vector<int>& out)
{
    size_t tmp = 0;
    EDLIB_AMD_HIP(select_slots_scratch_bytes(g.nslots, &tmp));
    EDLIB_AMD_HIP(d_selTmp_.ensure(tmp));
    EDLIB_AMD_HIP(g.d_list.ensure((size_t)g.nslots + 1));
    int* count = g.d_list.p + g.nslots;
    EDLIB_AMD_HIP(launch_select_open_slots(g.d_perm.p, g.d_total.p, g.d_qlen.p, cfg_.k, kDone, g.nslots, g.d_list.p, count,
                                           d_selTmp_.p, d_selTmp_.bytes(), stream_, g.mates));
    int n = 0;
    EDLIB_AMD_HIP(hipMemcpyAsync(&n, count, sizeof(int), hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    out.resize((size_t)n);
    if (n > 0) {
        EDLIB_AMD_HIP(hipMemcpyAsync(out.data(), g.d_list.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    }
    return 0;
}

// ------------------------------------------------------- exact k-mer seed filter (reads_seed.hip)

// k_f of a group: the largest k <= 16 whose k + 1 pieces of the shortest read hold at least kSeedQ symbols each and whose
// expected random exact hits per read on a uniform target, (k + 1) T / 4^L, stay at or below 1/8 (150-base reads against
// 5 Mb: k_f = 9, ten pieces of 15 symbols, 0.05 random windows per read).  -1: the group takes the banded first pass.
int Batch::seedThreshold(const ReadGroup& g, bool fullOnly) const
{
    const long long T = tlen(0);
    if (fullOnly || !banded_ || cfg_.mode != EDLIB_MODE_HW || syms_ != 4 || cfg_.additionalEqualitiesLength > 0 ||
        g.nwords > kMaxReadWords || chain_.in != nullptr || chain_.out != nullptr)
        return -1;
    // The index costs every run 0.5 ms at 5 Mb (measured: count 0.19, rocPRIM scan of the 4^12 counts 0.08, fill 0.23 ms), the
    // banded pass 888 ms per 5e12 read-columns: it pays from ~1e9 read-columns and ~600 reads at 5 Mb.  Smaller batches, and
    // targets shorter than 64 columns per query row, keep the banded pass.
    if (T < 64LL * 32 * g.nwords || g.nslots < 1024 || (long long)g.nslots * T < (1LL << 30)) return -1;
    int kf = -1;
    for (int k = 16; k >= 0 && kf < 0; --k) {
        const int L = g.mMin / (k + 1);
        if (L >= kSeedQ && (double)(k + 1) * (double)T <= std::ldexp(1.0, 2 * L) / 8.0) kf = k;
    }
    // a k_f below the banded pass's first threshold (8) would leave more reads to the full-height pass than that pass does
    // (short reads against long targets: 40 bases against 5 Mb give k_f = 1), unless the caller's k is no higher
    return (kf >= 0 && kf >= std::min(8, cfg_.k >= 0 ? cfg_.k : 8)) ? kf : -1;
}

// the buckets of the shared target: rebuilt in every run, as d_tpk_ is (a step does all of its target-dependent work)
int Batch::buildSeedIndex()
{
    const int T = tlen(0);
    EDLIB_AMD_HIP(d_seedCnt_.ensure((size_t)kSeedBuckets + 1));
    EDLIB_AMD_HIP(d_seedOff_.ensure((size_t)kSeedBuckets + 1));
    EDLIB_AMD_HIP(d_seedPos_.ensure((size_t)T));
    size_t tmp = 0;
    EDLIB_AMD_HIP(seed_index_scratch_bytes(&tmp));
    EDLIB_AMD_HIP(d_seedTmp_.ensure(tmp));
    scanTimerStart();
    EDLIB_AMD_HIP(launch_build_seed_index(d_tpk_.p, T, d_seedCnt_.p, d_seedOff_.p, d_seedPos_.p, d_seedTmp_.p,
                                          d_seedTmp_.bytes(), stream_));
    scanTimerStop();
    return 0;
}

// Pass 1 of a seed group at threshold k: every slot gets merge_segments_kernel's record (best or -1, the number of end
// locations, the first 16, the overflow flag) from its windows; the slots the filter hands back are scanned with the banded
// kernel over the whole target at the same threshold and merged through the slot map.
int Batch::runSeedPass(ReadGroup& g, int k)
{
    const int T = tlen(0);
    DevBuf<int> d_back;                                        // [nslots] handed-back slots, then their number
    EDLIB_AMD_HIP(d_back.alloc((size_t)g.nslots + 1));
    int* backCount = d_back.p + g.nslots;
    EDLIB_AMD_HIP(hipMemsetAsync(backCount, 0, sizeof(int), stream_));
    SeedArgs a{};
    a.peq = g.d_peq.p; a.qlen = g.d_qlen.p; a.perm = g.d_perm.p; a.tpk = d_tpk_.p; a.targetLength = T;
    a.seedOff = d_seedOff_.p; a.seedPos = d_seedPos_.p; a.nslots = g.nslots; a.k = k;
    a.best = g.d_best.p; a.total = g.d_total.p; a.pos = g.d_pos.p; a.flags = g.d_flags.p;
    a.backSlots = d_back.p; a.backCount = backCount; a.wordSteps = d_wordSteps_.p;
    scanTimerStart();
    EDLIB_AMD_HIP(launch_seed_verify(g.nwords, a, stream_));
    scanTimerStop();
    int nb = 0;
    EDLIB_AMD_HIP(hipMemcpyAsync(&nb, backCount, sizeof(int), hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    static const bool dbg = getenv("EDLIB_AMD_DEBUG") != nullptr;
    // (tests/test_gpu_seed_filter.py reads this line)
    if (dbg) fprintf(stderr, "[edlib_amd] seed pass nwords=%d k=%d: %d of %d slots handed back\n", g.nwords, k, nb, g.nslots);
    if (nb <= 0) return 0;
    int S2, segLen2, warm2;
    plan_segments(nb, T, EDLIB_MODE_HW, g.warm, 65536, S2, segLen2, warm2);
    const size_t items = (size_t)nb * S2;
    DevBuf<int> d_sb, d_sc, d_sp;
    EDLIB_AMD_HIP(d_sb.alloc(items)); EDLIB_AMD_HIP(d_sc.alloc(items)); EDLIB_AMD_HIP(d_sp.alloc(items * 8));
    if (scanGroup(g, EDLIB_MODE_HW, d_back.p, nb, k, g.d_kinit.p, S2, segLen2, warm2, d_sb.p, d_sc.p, d_sp.p, 8,
                  nullptr, nullptr)) return 1;
    EDLIB_AMD_HIP(launch_merge_segments(d_sb.p, d_sc.p, d_sp.p, S2, 8, nb, d_back.p, 16, g.d_best.p, g.d_total.p,
                                        g.d_pos.p, g.d_flags.p, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));            // temporaries die here
    return 0;
}

// Exact second pass for the (rare) slots with more end locations than the first pass keeps.  Their best score b is already
// exact.  Where every segment that holds b kept all of its hits (the merge's flag says so), the complete list is in the
// segment records and a gather copies it out.  The others are scanned again, "score <= b" selecting exactly the end
// locations: (a) a counting scan over fine segments gives the number of hits of every (slot, segment),
// (b) after a prefix sum the same scan writes them to their final place.  Fine segments keep
// the pass parallel (a handful of slots still fills the chip).
int Batch::runGroupExact(ReadGroup& g)
{
    const int T = tlen(0);
    const int mode = (cfg_.mode == EDLIB_MODE_HW || cfg_.mode == EDLIB_MODE_SHW) ? (int)cfg_.mode : (int)EDLIB_MODE_NW;
    const int kNoCap = 0x3fffffff;
    const size_t ns = (size_t)g.nslots;
    g.ovfSlots.clear(); g.ovfOff.assign(1, 0);
    if (mode == EDLIB_MODE_NW) return 0;
    // the flagged slots, ascending, with their flag and their number of end locations
    std::vector<int> recs;                                    // {slot, flag, total} each
    if (g.zeroCopy && !g.mates) {
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        for (size_t s = 0; s < ns; ++s)
            if (g.d_flags.p[s] && g.perm[s] >= 0) { recs.push_back((int)s); recs.push_back(g.d_flags.p[s]); recs.push_back(g.d_total.p[s]); }
    } else {
        size_t tmp = 0;
        EDLIB_AMD_HIP(select_slots_scratch_bytes(g.nslots, &tmp));
        EDLIB_AMD_HIP(d_selTmp_.ensure(tmp));
        EDLIB_AMD_HIP(g.d_list.ensure(ns + 1));
        int* count = g.d_list.p + ns;
        EDLIB_AMD_HIP(launch_select_flagged_slots(g.d_perm.p, g.d_flags.p, g.nslots, g.d_list.p, count,
                                                  d_selTmp_.p, d_selTmp_.bytes(), stream_, g.mates ? g.d_win.p : nullptr));
        int novf = 0;
        EDLIB_AMD_HIP(hipMemcpyAsync(&novf, count, sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        if (novf > 0) {
            DevBuf<int> d_recs;
            EDLIB_AMD_HIP(d_recs.alloc((size_t)novf * 3));
            EDLIB_AMD_HIP(launch_pick_slot_records(g.d_list.p, novf, g.d_flags.p, g.d_total.p, d_recs.p, stream_));
            recs.resize((size_t)novf * 3);
            EDLIB_AMD_HIP(hipMemcpyAsync(recs.data(), d_recs.p, recs.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
            EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
        }
    }
    const size_t no = recs.size() / 3;
    if (!no) return 0;
    // who is gathered from which records (lane of the scan that left them), who is scanned again
    std::vector<int> src(no, 0), at(no, -1);                  // 0: scan again, 1: the last level's records, 2: pass 1's
    std::vector<int> rescan;
    for (size_t i = 0; i < no; ++i) {
        const int s = recs[3 * i], f = recs[3 * i + 1];
        g.ovfSlots.push_back(s);
        if (f == kOvfGatherLevel && g.lvValid) {
            const auto it = std::lower_bound(g.lvMap.begin(), g.lvMap.end(), s);
            if (it != g.lvMap.end() && *it == s) { src[i] = 1; at[i] = (int)(it - g.lvMap.begin()); }
        } else if (f == kOvfGatherGroup) { src[i] = 2; at[i] = s; }
        if (!src[i]) { at[i] = (int)rescan.size(); rescan.push_back(s); }
    }
    const size_t nr = rescan.size();
    int S2 = 1, segLen2 = 0, warm2 = 0;
    DevBuf<int> d_map, d_caps, d_sb, d_sc; DevBuf<long long> d_off;
    std::vector<int> cnts;
    if (nr) {
        // (a handful of slots is a handful of waves per segment: the pass takes what ONE wave takes for its segment, so the
        // segments go down to four warm-ups -- 18 slots of a 16,384-read batch: 2 x 0.83 ms at 4,112 columns)
        plan_segments((int)nr, T, mode, g.warm, 16384, S2, segLen2, warm2, nr <= 256 ? 1024 : 4096);
        const size_t items = nr * (size_t)S2;
        EDLIB_AMD_HIP(d_map.alloc(nr)); EDLIB_AMD_HIP(d_sb.alloc(items)); EDLIB_AMD_HIP(d_sc.alloc(items));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_map.p, rescan.data(), nr * sizeof(int), hipMemcpyHostToDevice, stream_));
        // (a) count; threshold = the exact best (d_best), so the band is as narrow as it gets
        if (scanGroup(g, mode, d_map.p, (int)nr, kNoCap, g.d_best.p, S2, segLen2, warm2,
                      d_sb.p, d_sc.p, d_sb.p /*unused*/, 0, nullptr, nullptr)) return 1;
        cnts.resize(items);
        EDLIB_AMD_HIP(hipMemcpyAsync(cnts.data(), d_sc.p, items * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    }
    // the lists in slot order: a gathered slot takes the merge's total, a rescanned one what its segments counted
    std::vector<long long> offs(nr * (size_t)S2);
    std::vector<int> gIdx[2], gLim[2]; std::vector<long long> gOff[2];
    long long acc = 0;
    g.ovfOff.assign(no + 1, 0);
    for (size_t i = 0; i < no; ++i) {
        if (src[i]) {
            const int w = src[i] - 1, n = std::max(0, recs[3 * i + 2]);
            gIdx[w].push_back(at[i]); gOff[w].push_back(acc); gLim[w].push_back(n);
            acc += n;
        } else {
            const size_t r = (size_t)at[i];
            for (int sg = 0; sg < S2; ++sg) { offs[r * S2 + sg] = acc; acc += cnts[r * S2 + sg]; }
        }
        g.ovfOff[i + 1] = acc;
    }
    EDLIB_AMD_HIP(g.d_ovfPool.ensure((size_t)std::max<long long>(acc, 1)));
    DevBuf<int> d_gi[2], d_gl[2]; DevBuf<long long> d_go[2];
    for (int w = 0; w < 2; ++w) {
        const size_t n = gIdx[w].size();
        if (!n) continue;
        EDLIB_AMD_HIP(d_gi[w].alloc(n)); EDLIB_AMD_HIP(d_gl[w].alloc(n)); EDLIB_AMD_HIP(d_go[w].alloc(n));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_gi[w].p, gIdx[w].data(), n * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_gl[w].p, gLim[w].data(), n * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_go[w].p, gOff[w].data(), n * sizeof(long long), hipMemcpyHostToDevice, stream_));
        if (w == 0)
            EDLIB_AMD_HIP(launch_gather_segments(g.d_lvBest.p, g.d_lvCnt.p, g.d_lvPos.p, g.lvS, g.lvCap, (int)n,
                                                 d_gi[w].p, d_go[w].p, d_gl[w].p, g.d_ovfPool.p, stream_));
        else
            EDLIB_AMD_HIP(launch_gather_segments(g.d_segBest.p, g.d_segCnt.p, g.d_segPos.p, g.numSegments, 8, (int)n,
                                                 d_gi[w].p, d_go[w].p, d_gl[w].p, g.d_ovfPool.p, stream_));
    }
    if (nr) {
        const size_t items = nr * (size_t)S2;
        EDLIB_AMD_HIP(d_caps.alloc(items)); EDLIB_AMD_HIP(d_off.alloc(items));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_caps.p, cnts.data(), items * sizeof(int), hipMemcpyHostToDevice, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(d_off.p, offs.data(), items * sizeof(long long), hipMemcpyHostToDevice, stream_));
        // (b) write
        if (scanGroup(g, mode, d_map.p, (int)nr, kNoCap, g.d_best.p, S2, segLen2, warm2,
                      d_sb.p, d_sc.p, g.d_ovfPool.p, 0, d_off.p, d_caps.p)) return 1;
    }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));                    // temporaries die here
    static const bool dbg = getenv("EDLIB_AMD_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[edlib_amd] exact pass nwords=%d: %zu gathered, %zu rescanned\n", g.nwords, no - nr, nr);
    stats.overflow_units += (int)no;
    return 0;
}

// ------------------------------------------------------- hit-list read batches (reads_hits.hip)

// The banded HITS scan of `nlanes` lanes of a group (all of its slots, or the slots of d_slotmap) at the caller's k
int Batch::hitsScanBanded(ReadGroup& g, int slotBase, const int* d_slotmap, int nlanes, int numSegments, int segLen, int warm)
{
    ReadScanArgs a{};
    a.peq = g.d_peq.p; a.tpk = d_tpk_.p; a.trows = d_trows_.p; a.targetLength = tlen(0);
    a.qlen = g.d_qlen.p; a.kinit = g.d_kinit.p; a.slotmap = d_slotmap; a.nlanes = nlanes;
    a.numSegments = numSegments; a.segLen = segLen; a.warm = warm;
    a.cap = 1;                                                 // (a live lane; the records of the other scans are not written)
    a.kcap = 0x3fffffff; a.wordSteps = d_wordSteps_.p;
    a.hits = hitList_.list(); a.slotBase = slotBase;
    scanTimerStart();
    EDLIB_AMD_HIP(launch_scan_reads_hits(g.nwords, syms_, a, stream_));
    scanTimerStop();
    return 0;
}

// One group: the seed pass where the seed filter is exact at k (its hand-backs through the banded scan), else the banded scan
int Batch::scanGroupHits(ReadGroup& g, int slotBase)
{
    const int T = tlen(0);
    const int kSeed = seedThreshold(g, false);
    if (kSeed < 0 || cfg_.k > kSeed) return hitsScanBanded(g, slotBase, nullptr, g.nslots, g.numSegments, g.segLen, g.warm);
    DevBuf<int> d_back;                                        // [nslots] handed-back slots, then their number
    EDLIB_AMD_HIP(d_back.alloc((size_t)g.nslots + 1));
    int* backCount = d_back.p + g.nslots;
    EDLIB_AMD_HIP(hipMemsetAsync(backCount, 0, sizeof(int), stream_));
    SeedArgs a{};
    a.peq = g.d_peq.p; a.qlen = g.d_qlen.p; a.perm = g.d_perm.p; a.tpk = d_tpk_.p; a.targetLength = T;
    a.seedOff = d_seedOff_.p; a.seedPos = d_seedPos_.p; a.nslots = g.nslots; a.k = cfg_.k;
    a.backSlots = d_back.p; a.backCount = backCount; a.wordSteps = d_wordSteps_.p;
    a.hits = hitList_.list(); a.slotBase = slotBase;
    scanTimerStart();
    EDLIB_AMD_HIP(launch_seed_verify_hits(g.nwords, a, stream_));
    scanTimerStop();
    int nb = 0;
    EDLIB_AMD_HIP(hipMemcpyAsync(&nb, backCount, sizeof(int), hipMemcpyDeviceToHost, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    static const bool dbg = getenv("EDLIB_AMD_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[edlib_amd] seed hits pass nwords=%d k=%d: %d of %d slots handed back\n", g.nwords, cfg_.k, nb, g.nslots);
    if (nb > 0) {
        int S2, segLen2, warm2;
        plan_segments(nb, T, EDLIB_MODE_HW, g.warm, 65536, S2, segLen2, warm2);
        if (hitsScanBanded(g, slotBase, d_back.p, nb, S2, segLen2, warm2)) return 1;
        EDLIB_AMD_HIP(hipStreamSynchronize(stream_));          // d_back dies here
    }
    return 0;
}

int Batch::runReadHits()
{
    const int T = tlen(0);
    stats.path |= 1;
    if (!d_hitSlotUnit_.p) {
        // the batch-wide slot table: the groups' slots one after the other, then a slot per empty unit
        std::vector<int> slotUnit;
        for (auto& gp : groups_) slotUnit.insert(slotUnit.end(), gp->perm.begin(), gp->perm.end());
        // empty sequences are answered here: an empty read hits once, the whole target at distance 0; an empty target has no hit
        for (int u : emptyUnits_) {
            if (T > 0 && qlen(u) == 0) {
                hostHits_.key.push_back((unsigned long long)(uint32_t)slotUnit.size() << 32);
                hostHits_.val[0].push_back(T - 1); hostHits_.val[1].push_back(0); hostHits_.val[2].push_back(0); hostHits_.val[3].push_back(T);
            }
            slotUnit.push_back(u);
        }
        EDLIB_AMD_HIP(d_hitSlotUnit_.alloc(slotUnit.size()));
        if (!slotUnit.empty())
            EDLIB_AMD_HIP(hipMemcpy(d_hitSlotUnit_.p, slotUnit.data(), slotUnit.size() * sizeof(int), hipMemcpyHostToDevice));
        EDLIB_AMD_HIP(d_hitTotal_.alloc(1));
        // (2^31 - 1 entries: the finish kernels index with int)
        hitList_.configure("hit-list read batch", "runs", 4, 31, false, kReadHitsExtraBytes);
        if (hitList_.size((size_t)n_, std::max<long long>(1LL << 20, n_), stream_)) return 1;
    }
    if (packTarget()) return 1;
    bool seed = false;
    for (auto& gp : groups_) { const int ks = seedThreshold(*gp, false); seed = seed || (ks >= 0 && cfg_.k <= ks); }
    if (seed && buildSeedIndex()) return 1;
    for (auto& gp : groups_)
        EDLIB_AMD_HIP(launch_build_peq_reads(gp->nwords, syms_, d_qpool_.p, d_qoff_.p, gp->d_perm.p, gp->nslots, d_eqtbl_.p,
                                             d_presence_.p, cfg_.k, gp->d_peq.p, gp->d_qlen.p, gp->d_kinit.p,
                                             gp->d_alphaExtra.p, stream_));
    auto scanGroups = [&]() -> int {
        int slotBase = 0;
        for (auto& gp : groups_) {
            if (scanGroupHits(*gp, slotBase)) return 1;
            slotBase += gp->nslots;
        }
        return 0;
    };
    EDLIB_AMD_HIP(hitList_.reset(stream_));
    if (scanGroups() || hitList_.settle(hostHits_, stream_, scanGroups)) return 1;
    unsigned long long* total = hitList_.pinnedWord();
    hitList_.outN = 0;
    if (hitList_.n > 0) {
        EDLIB_AMD_HIP(launch_read_hits_finish(hitList_, d_hitSlotUnit_.p, n_, d_hitTotal_.p, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(total, d_hitTotal_.p, sizeof(long long), hipMemcpyDeviceToHost, stream_));
    } else EDLIB_AMD_HIP(hipMemsetAsync(hitList_.off(), 0, ((size_t)n_ + 1) * sizeof(long long), stream_));
    if (banded_ && !groups_.empty() && enqueueWordSteps()) return 1;
    if (endRun()) return 1;
    if (hitList_.n > 0) hitList_.outN = (long long)*total;
    stats.algo_bytes = 0;
    hitsHaveRun_ = true;
    return 0;
}

// The hits of the last Run, as one block in pinned memory: the unit offsets, then the five arrays
int Batch::hitsView(EdlibAmdReadHits* out)
{
    if (!hits_) {
        set_error("edlibAmdBatchSharedHits: not a hit-list read batch (create it with edlibAmdBatchCreateSharedHits)");
        return 1;
    }
    if (!hitsHaveRun_) { set_error("hit-list read batch: no results (Run it first)"); return 1; }
    pool_quarantine(false);
    DeviceGuard guard(device_);
    EDLIB_AMD_HIP(guard.status);
    const long long* off = nullptr;
    const int* l = nullptr;
    if (hitList_.fetch(5, stream_, &off, &l)) return 1;
    memset(out, 0, sizeof *out);
    out->numUnits = n_; out->numHits = hitList_.outN;
    out->unitOffsets = off;
    const size_t n = (size_t)hitList_.outN;
    out->firstEnd = l; out->lastEnd = l + n; out->editDistance = l + 2 * n; out->endLocation = l + 3 * n; out->numLocations = l + 4 * n;
    return 0;
}

// the shared target in the forms the reads-per-lane kernels read (once per run; the work counter of the banded kernel)
int Batch::packTarget()
{
    if (groups_.empty() && longUnits_.empty()) return 0;
    const int T = tlen(0);
    EDLIB_AMD_HIP(hipMemsetAsync(d_wordSteps_.p, 0, sizeof(unsigned long long), stream_));
    if (syms_ == 4) EDLIB_AMD_HIP(launch_pack_target_2bit(d_tpool_.p, d_tlut_.p, T, d_tpk_.p, stream_));
    if (banded_) EDLIB_AMD_HIP(launch_pack_target_rows(d_tpool_.p, d_tlut_.p, T, d_trows_.p, (int)d_trows_.n, stream_));
    return 0;
}

int Batch::collectReads(std::vector<UnitResult>& res)
{
    if (groups_.empty()) return 0;
    for (auto& gp : groups_) if (collectGroup(*gp, res)) return 1;
    readsCollected_ = true;
    return 0;
}

// D2H of one group's merged per-slot results + the result semantics of its units
int Batch::collectGroup(ReadGroup& g, std::vector<UnitResult>& res)
{
    const int T = tlen(0);
    const int mode = (cfg_.mode == EDLIB_MODE_HW || cfg_.mode == EDLIB_MODE_SHW) ? (int)cfg_.mode : (int)EDLIB_MODE_NW;
    const size_t ns = (size_t)g.nslots;
    // merged per-slot results: read in place when they already live in pinned host memory (small groups), else
    // downloaded into pinned staging (a copy into pageable memory runs at a fraction of the link rate: 64 bytes
    // per read were 20 ms per 1M reads)
    std::vector<int> ovfPos((size_t)g.ovfOff.back());
    PinBuf stage;
    const int *best, *total, *extra, *pos;
    if (g.zeroCopy) {                          // run() synchronised the stream
        best = g.d_best.p; total = g.d_total.p; extra = g.d_alphaExtra.p; pos = g.d_pos.p;
    } else {
        EDLIB_AMD_HIP(stage.alloc(ns * 19 * sizeof(int)));
        int* h = reinterpret_cast<int*>(stage.p);
        EDLIB_AMD_HIP(hipMemcpyAsync(h, g.d_best.p, ns * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(h + ns, g.d_total.p, ns * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(h + 2 * ns, g.d_alphaExtra.p, ns * sizeof(int), hipMemcpyDeviceToHost, stream_));
        EDLIB_AMD_HIP(hipMemcpyAsync(h + 3 * ns, g.d_pos.p, ns * 16 * sizeof(int), hipMemcpyDeviceToHost, stream_));
        best = h; total = h + ns; extra = h + 2 * ns; pos = h + 3 * ns;
    }
    if (!ovfPos.empty())
        EDLIB_AMD_HIP(hipMemcpyAsync(ovfPos.data(), g.d_ovfPool.p, ovfPos.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
    PinBuf winStage;
    const int* win = nullptr;                  // both strands: what every mate pair reports
    if (g.mates) {
        EDLIB_AMD_HIP(winStage.alloc(ns / 2 * sizeof(int)));
        EDLIB_AMD_HIP(hipMemcpyAsync(winStage.p, g.d_win.p, ns / 2 * sizeof(int), hipMemcpyDeviceToHost, stream_));
        win = reinterpret_cast<const int*>(winStage.p);
    }
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    size_t oi = 0;
    for (size_t s = 0; s < ns; ++s) {
        const int u = g.perm[s];
        if (u < 0) continue;
        UnitResult& r = res[u];
        if (deferReadsReset_) blank_record(r);
        if (win) {
            const int w = win[s >> 1];
            if (!(s & 1)) setStrand(u >> 1, w);
            // the mate is reported: this record stays blank (its slot may be pruned, its list above 16 was never made)
            if ((w & kStrandReverse) != (int)(s & 1)) { blank_record(r); continue; }
        }
        r.alphabetLength = tab_.sigmaT + extra[s];
        const int m = qlen(u);
        if (mode == EDLIB_MODE_HW || mode == EDLIB_MODE_SHW) {
            if (oi < g.ovfSlots.size() && g.ovfSlots[oi] == (int)s) {
                finalize_semiglobal(r, cfg_.k, m, best[s], ovfPos.data() + g.ovfOff[oi], g.ovfOff[oi + 1] - g.ovfOff[oi]);
                ++oi;
            } else {
                finalize_semiglobal(r, cfg_.k, m, best[s], pos + s * 16, best[s] < 0 ? 0 : total[s]);
            }
        } else {
            finalize_global(r, cfg_.k, (int)cfg_.mode, T, best[s]);
        }
    }
    return 0;
}


}  // namespace edlib_amd
