// engine_lanes.hip -- what the cross, self and window engines keep alike (engine_lanes.hpp), and the pieces of an init
// that Batch::init shares with them.
#include "engine_lanes.hpp"

#include <algorithm>
#include <cstring>

namespace edlib_amd {

int check_device(int device)
{
    const int ndev = device_count();
    if (ndev == 0) { set_error("no usable HIP device (this library has no CPU fallback)"); return 1; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return 1; }
    return 0;
}

void keep_config(const EdlibAlignConfig& cfg, EdlibAlignConfig& kept, std::vector<EdlibEqualityPair>& eqs)
{
    kept = cfg;
    if (cfg.additionalEqualities && cfg.additionalEqualitiesLength > 0)
        eqs.assign(cfg.additionalEqualities, cfg.additionalEqualities + cfg.additionalEqualitiesLength);
    kept.additionalEqualities = eqs.empty() ? nullptr : eqs.data();
    kept.additionalEqualitiesLength = (int)eqs.size();
}

int copy_offsets(const long long* in, int n, const char* what, std::vector<long long>& out)
{
    out.assign((size_t)n + 1, 0);
    if (in) out.assign(in, in + n + 1);
    for (int i = 0; i < n; ++i)
        if (out[i + 1] < out[i] || out[i + 1] - out[i] > 0x7fffffffLL) { set_error("bad %s offsets", what); return 1; }
    return 0;
}

std::string with_commas(long long v)
{
    std::string s = std::to_string(v);
    for (int i = (int)s.size() - 3; i > 0; i -= 3) s.insert((size_t)i, ",");
    return s;
}

void PairPool::add(const char* q, long long qn, bool reverse, const char* t, long long tn)
{
    if (!reverse) qp.insert(qp.end(), q, q + qn);
    else
        for (long long j = qn - 1; j >= 0; --j) qp.push_back((char)complement_byte((uint8_t)q[j]));
    tp.insert(tp.end(), t, t + tn);
    qo.push_back((long long)qp.size()); to.push_back((long long)tp.size());
}

int PairPool::init(Batch& b, const EdlibAlignConfig& cfg, int device)
{
    if (qp.empty()) qp.push_back(0);
    if (tp.empty()) tp.push_back(0);
    return b.init(qp.data(), qo.data(), (int)size(), tp.data(), to.data(), (int)size(), cfg, device);
}

void LaneEngine::closeStream()
{
    DeviceGuard guard(device_);
    if (stream_) { (void)hipStreamSynchronize(stream_); pool_stream_release(stream_); }
}

int LaneEngine::openStream()
{
    EDLIB_AMD_HIP(pool_stream(&stream_));
    EDLIB_AMD_HIP(evScan0_.create()); EDLIB_AMD_HIP(evScan1_.create());
    return 0;
}

int LaneEngine::uploadQueries(const char* queries, const std::vector<long long>& qoff, bool strands)
{
    const int nq = (int)qoff.size() - 1;
    const long long qb = qoff[0], qbytes = qoff[nq] - qb;
    std::vector<long long> qoffR(qoff);
    for (auto& v : qoffR) v -= qb;
    if (!strands) {
        EDLIB_AMD_HIP(d_qpool_.alloc((size_t)qbytes + 16)); EDLIB_AMD_HIP(d_qoff_.alloc((size_t)nq + 1));
        if (qbytes) EDLIB_AMD_HIP(hipMemcpy(d_qpool_.p, queries + qb, (size_t)qbytes, hipMemcpyHostToDevice));
        EDLIB_AMD_HIP(hipMemcpy(d_qoff_.p, qoffR.data(), ((size_t)nq + 1) * sizeof(long long), hipMemcpyHostToDevice));
    } else {
        // the caller's pool goes up as it is; query i and its reverse complement are written from it on the device as
        // the entries 2i and 2i + 1 of a pool twice its size
        if (make_strand_pool(queries + qb, qoffR.data(), nq, d_qpool_, d_qoff_, stream_)) return 1;
    }
    EDLIB_AMD_HIP(d_eqtbl_.alloc(256)); EDLIB_AMD_HIP(d_presence_.alloc(8));
    EDLIB_AMD_HIP(hipMemcpy(d_eqtbl_.p, tab_.eqtbl, 512, hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(hipMemcpy(d_presence_.p, tab_.presence, 32, hipMemcpyHostToDevice));
    return 0;
}

int LaneEngine::packTargets(const uint8_t* d_pool, const long long* d_off, const std::vector<int>& order,
                            const std::vector<int>& len)
{
    const int n = (int)order.size();
    std::vector<long long> tdw(n);
    long long dw = 0;
    for (int i = 0; i < n; ++i) { tdw[i] = dw; dw += (len[i] + 7) / 8; }
    DevBuf<uint8_t> d_tlut;
    EDLIB_AMD_HIP(d_tpk_.alloc((size_t)std::max(dw, 1LL)));
    EDLIB_AMD_HIP(d_tdw_.alloc(n)); EDLIB_AMD_HIP(d_tperm_.alloc(n)); EDLIB_AMD_HIP(d_tlut.alloc(256));
    EDLIB_AMD_HIP(hipMemcpy(d_tdw_.p, tdw.data(), n * sizeof(long long), hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(hipMemcpy(d_tperm_.p, order.data(), n * sizeof(int), hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(hipMemcpy(d_tlut.p, tab_.tlut, 256, hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(launch_pack_cross_targets(d_pool, d_off, d_tperm_.p, d_tdw_.p, n, d_tlut.p, d_tpk_.p, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    return 0;
}

int LaneEngine::packHostTargets(const char* pool, const std::vector<long long>& off, const std::vector<int>& order,
                                const std::vector<int>& len)
{
    const long long tb = off.front(), tbytes = off.back() - tb;
    std::vector<long long> offR(off);
    for (auto& v : offR) v -= tb;
    DevBuf<uint8_t> d_traw; DevBuf<long long> d_toff;
    EDLIB_AMD_HIP(d_traw.alloc((size_t)tbytes + 16)); EDLIB_AMD_HIP(d_toff.alloc(offR.size()));
    if (tbytes) EDLIB_AMD_HIP(hipMemcpy(d_traw.p, pool + tb, (size_t)tbytes, hipMemcpyHostToDevice));
    EDLIB_AMD_HIP(hipMemcpy(d_toff.p, offR.data(), offR.size() * sizeof(long long), hipMemcpyHostToDevice));
    return packTargets(d_traw.p, d_toff.p, order, len);
}

int LaneEngine::allocGroup(LaneGroup& g, const std::vector<int>& perm)
{
    g.slots = (int)perm.size();
    const size_t blocks = (size_t)(g.slots + 63) / 64;
    EDLIB_AMD_HIP(g.d_perm.alloc(g.slots)); EDLIB_AMD_HIP(g.d_qlen.alloc(g.slots));
    EDLIB_AMD_HIP(g.d_kinit.alloc(g.slots)); EDLIB_AMD_HIP(g.d_alpha.alloc(g.slots));
    EDLIB_AMD_HIP(g.d_peq.alloc(blocks * syms_ * g.words * 64));
    EDLIB_AMD_HIP(hipMemcpy(g.d_perm.p, perm.data(), g.slots * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

int LaneEngine::buildPeq(LaneGroup& g)
{
    EDLIB_AMD_HIP(launch_build_peq_reads(g.words, syms_, d_qpool_.p, d_qoff_.p, g.d_perm.p, g.slots, d_eqtbl_.p, d_presence_.p,
                                         cfg_.k, g.d_peq.p, g.d_qlen.p, g.d_kinit.p, g.d_alpha.p, stream_));
    return 0;
}

int LaneEngine::beginRun(hipError_t guardStatus, std::initializer_list<PinnedPart*> parts)
{
    EDLIB_AMD_HIP(guardStatus);
    haveRun_ = false;
    for (PinnedPart* p : parts) p->fetched = false;
    const long long cells = stats.cells;
    stats = EdlibAmdBatchStats{};
    stats.cells = cells;
    return 0;
}

int LaneEngine::endRun(std::chrono::steady_clock::time_point t0, bool scanned)
{
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    if (scanned) {
        float ms = 0.f;
        EDLIB_AMD_HIP(hipEventElapsedTime(&ms, evScan0_.e, evScan1_.e));
        stats.scan_ms = ms;
    }
    stats.algo_bytes = 0;
    stats.run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    haveRun_ = true;
    return 0;
}

int LaneEngine::fetchParts(std::initializer_list<WantedPart> wants)
{
    for (const WantedPart& w : wants)
        if (w.asked) EDLIB_AMD_HIP(w.part->fetch(w.dev, w.bytes, stream_));
    EDLIB_AMD_HIP(hipStreamSynchronize(stream_));
    for (const WantedPart& w : wants)
        if (w.asked) w.part->fetched = true;
    return 0;
}

int LaneEngine::readCells(Batch& b, size_t n, int* vals, const char* engine)
{
    EdlibAmdResultsView v{};
    if (b.resultsView(&v)) return 1;
    for (size_t i = 0; i < n; ++i) {
        if (v.status[i] != EDLIB_STATUS_OK) { set_error("%s batch: an internal alignment failed", engine); return 1; }
        vals[3 * i] = v.editDistance[i];
        vals[3 * i + 1] = v.numLocations[i];
        vals[3 * i + 2] = v.numLocations[i] > 0 ? v.endLocations[v.locOffsets[i]] : -1;
    }
    return 0;
}

void LaneEngine::addSessionStats(Batch& b, bool wordSteps)
{
    b.finishStats();
    const EdlibAmdBatchStats& s = b.stats;
    if (wordSteps) stats.word_steps += s.word_steps;
    stats.scan_launches += s.scan_launches;
    stats.path |= s.path; stats.overflow_units += s.overflow_units; stats.wide_retries += s.wide_retries;
}

}  // namespace edlib_amd
