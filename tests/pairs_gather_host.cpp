// pairs_gather_host.cpp -- TEST INFRASTRUCTURE: the device code of the pools gather (edlib_amd/csrc/pairs_gather_core.hpp)
// compiled for the host, the destination runs walked one by one in the kernel's order: block, thread, the block's pair
// range, the thread's pair, the run, the store.  Built by tests/test_pairs_gather_model.py with g++ into
// build/libpairs_gather_host.so; with -DPAIRS_GATHER_MAIN it is a program of its own that gathers a small grid from
// exactly sized heap blocks and compares it with byte-wise slicing (the sanitizer build).  Never linked into the product.
#include "../edlib_amd/csrc/pairs_gather_core.hpp"

#include <string.h>

using namespace edlib_amd::pairs_gather;

// the kernel's wave search, the ballot counted lane by lane
static int find_pair_wave(const long long* off, int lo, int hi, long long pos)
{
    while (lo < hi) narrow(lo, hi, count_probes(off, lo, hi, pos));
    return lo;
}

// the two searches by themselves: the largest p in [lo, hi] with off[p] <= pos
extern "C" int pairs_gather_host_find(const long long* off, int lo, int hi, long long pos, int wave)
{
    return wave ? find_pair_wave(off, lo, hi, pos) : find_pair(off, lo, hi, pos);
}

// the kernel's store: 16 bytes where the pool (total + 16 bytes) has them, its last bytes otherwise
static void store_run(uint8_t* pool, long long d0, long long total, const Run& r)
{
    const long long left = total + 16 - d0;
    uint8_t b[kRun];
    for (int j = 0; j < kRun; ++j) b[j] = (uint8_t)(r.w[j >> 3] >> (8 * (j & 7)));
    memcpy(pool + d0, b, left >= kRun ? (size_t)kRun : (size_t)left);
}

// Both pools of n >= 1 pairs (qout: qoff[n] + 16 bytes, tout: toff[n] + 16 bytes).  Returns 0.
extern "C" int pairs_gather_host(const uint32_t* pack, long long packDwords, const uint8_t* idToByte,
                                 const uint32_t* qpool, long long qpoolDwords, const long long* srcOff, int stranded,
                                 const uint8_t* comp, int n, const long long* qoff, const long long* toff,
                                 const int* pairQuery, const int* pairStart, const uint8_t* pairStrand,
                                 uint8_t* qout, uint8_t* tout)
{
    uint16_t tab2[256];
    for (int c = 0; c < 256; ++c) tab2[c] = (uint16_t)(idToByte[c & 15] | idToByte[c >> 4] << 8);
    TargetSource ts{pack, packDwords, pairStart};
    QuerySource qs{qpool, qpoolDwords, srcOff, stranded, pairQuery, pairStrand};
    for (int pool = 0; pool < 2; ++pool) {
        const long long* off = pool ? qoff : toff;
        const long long total = off[n];
        const long long blocks = (total + 16 + kBlockBytes - 1) / kBlockBytes;
        for (long long b = 0; b < blocks; ++b)
            for (int t = 0; t < kBlockThreads; ++t) {
                const long long d0 = (b * kBlockThreads + t) * kRun;
                if (d0 >= total + 16) continue;
                Run r; r.w[0] = 0; r.w[1] = 0;
                if (d0 < total) {
                    const int lo = find_pair_wave(off, 0, n - 1, block_first(total, b));
                    const int hi = find_pair_wave(off, lo, block_far(lo, n), block_last(total, b));
                    const int p = find_pair(off, lo, hi, d0);
                    r = pool ? query_run(d0, total, p, off, qs, comp) : target_run(d0, total, p, off, ts, tab2);
                }
                store_run(pool ? qout : tout, d0, total, r);
            }
    }
    return 0;
}

#if defined(PAIRS_GATHER_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static uint8_t comp_of(uint8_t b)
{
    static const char from[] = "ATUCGRYKMBVDH", to[] = "TAAGCYRMKVBHD";
    const bool lower = b >= 'a' && b <= 'z';
    const uint8_t up = lower ? (uint8_t)(b - 32) : b;
    for (int i = 0; from[i]; ++i)
        if (up == (uint8_t)from[i]) return lower ? (uint8_t)(to[i] + 32) : (uint8_t)to[i];
    return b;
}

int main()
{
    unsigned seed = 12345;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    const uint8_t comp_alpha[] = "ACGTNacgtnUuRYKMBVDHSW";
    uint8_t comp[256];
    for (int b = 0; b < 256; ++b) comp[b] = comp_of((uint8_t)b);
    int failures = 0;
    for (int sigma : {1, 4, 5, 16})
        for (int stranded = 0; stranded < 2; ++stranded) {
            // the target: sigma symbols, codes as a pack would hold them
            const int T = 1237;
            uint8_t ids[16];
            for (int i = 0; i < 16; ++i) ids[i] = (uint8_t)(i < sigma ? (i % 3 == 2 ? 128 + 7 * i : 'A' + i) : 0);
            std::vector<uint8_t> target(T);
            for (int j = 0; j < T; ++j) target[j] = ids[sigma == 16 && j % 5 == 0 ? 15 : (int)(rnd() % sigma)];
            const long long ndw = (T + 7) / 8;
            uint32_t* pack = (uint32_t*)calloc((size_t)ndw, 4);
            for (int j = 0; j < T; ++j) {
                int code = 0;
                while (ids[code] != target[j]) ++code;
                pack[j >> 3] |= (uint32_t)code << (4 * (j & 7));
            }
            // the queries
            const int lens[] = {1, 2, 3, 4, 5, 31, 32, 33, 150, 255, 256};
            const int nq = (int)(sizeof lens / sizeof lens[0]);
            std::vector<std::vector<uint8_t>> qs(nq);
            std::vector<long long> srcOff;
            std::vector<uint8_t> poolBytes;
            for (int q = 0; q < nq; ++q) {
                qs[q].resize(lens[q]);
                for (auto& c : qs[q]) c = comp_alpha[rnd() % (sizeof comp_alpha - 1)];
                srcOff.push_back((long long)poolBytes.size());
                poolBytes.insert(poolBytes.end(), qs[q].begin(), qs[q].end());
                if (stranded) {
                    srcOff.push_back((long long)poolBytes.size());
                    for (int j = lens[q] - 1; j >= 0; --j) poolBytes.push_back(comp_of(qs[q][j]));
                }
            }
            srcOff.push_back((long long)poolBytes.size());
            const long long qdw = ((long long)poolBytes.size() + 16) / 4;
            uint32_t* qpool = (uint32_t*)calloc((size_t)qdw, 4);
            memcpy(qpool, poolBytes.data(), poolBytes.size());
            // the pairs: every phase x a few lengths, the target's two ends, both strands
            std::vector<int> pq, ps, pl; std::vector<uint8_t> pst;
            const int wl[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 400};
            int i = 0;
            for (int phase = 0; phase < 8; ++phase)
                for (int L : wl) {
                    pq.push_back(i % nq); pst.push_back((uint8_t)((i / nq) & 1));
                    ps.push_back(8 * (int)(rnd() % 90) + phase); pl.push_back(L); ++i;
                }
            pq.push_back(0); pst.push_back(1); ps.push_back(0); pl.push_back(T);
            pq.push_back(10); pst.push_back(1); ps.push_back(T - 5); pl.push_back(5);
            const int n = (int)pq.size();
            std::vector<long long> qoff(n + 1, 0), toff(n + 1, 0);
            for (int p = 0; p < n; ++p) { qoff[p + 1] = qoff[p] + lens[pq[p]]; toff[p + 1] = toff[p] + pl[p]; }
            uint8_t* qout = (uint8_t*)malloc((size_t)qoff[n] + 16);
            uint8_t* tout = (uint8_t*)malloc((size_t)toff[n] + 16);
            memset(qout, 0xEE, (size_t)qoff[n] + 16); memset(tout, 0xEE, (size_t)toff[n] + 16);
            pairs_gather_host(pack, ndw, ids, qpool, qdw, srcOff.data(), stranded, comp, n, qoff.data(), toff.data(),
                              pq.data(), ps.data(), pst.data(), qout, tout);
            for (int p = 0; p < n; ++p) {
                for (int j = 0; j < pl[p]; ++j)
                    if (tout[toff[p] + j] != target[ps[p] + j]) { ++failures; break; }
                const std::vector<uint8_t>& q = qs[pq[p]];
                for (int j = 0; j < (int)q.size(); ++j)
                    if (qout[qoff[p] + j] != (pst[p] ? comp_of(q[q.size() - 1 - j]) : q[j])) { ++failures; break; }
            }
            for (int j = 0; j < 16; ++j)
                if (qout[qoff[n] + j] || tout[toff[n] + j]) { ++failures; break; }
            free(pack); free(qpool); free(qout); free(tout);
        }
    printf("pairs_gather_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
#endif
