// pairs_gather_cells_host.cpp -- TEST INFRASTRUCTURE: the device code that gathers a pair batch's target pool from a cross
// batch's pack of many targets (edlib_amd/csrc/pairs_gather_core.hpp: cell_base, target_run_cells) compiled for the host,
// the plan and the destination runs walked one by one in the kernels' order: the pair's base; block, thread, the block's
// pair range, the thread's pair, the run, the store.  Built by tests/test_pairs_gather_cells_model.py with g++ into
// build/libpairs_gather_cells_host.so; with -DPAIRS_GATHER_MAIN it is a program of its own that gathers a small grid from
// exactly sized heap blocks and compares it with byte-wise slicing (the sanitizer build).  Never linked into the product.
#include "../edlib_amd/csrc/pairs_gather_core.hpp"

#include <string.h>

using namespace edlib_amd::pairs_gather;

static int find_pair_wave(const long long* off, int lo, int hi, long long pos)
{
    while (lo < hi) narrow(lo, hi, count_probes(off, lo, hi, pos));
    return lo;
}

// the kernel's store: 16 bytes where the pool (total + 16 bytes) has them, its last bytes otherwise
static void store_run_words(uint8_t* pool, long long d0, long long total, uint64_t w0, uint64_t w1)
{
    const long long left = total + 16 - d0;
    uint8_t b[kRun];
    for (int j = 0; j < kRun; ++j) b[j] = (uint8_t)((j < 8 ? w0 : w1) >> (8 * (j & 7)));
    memcpy(pool + d0, b, left >= kRun ? (size_t)kRun : (size_t)left);
}

// The target pool of n >= 1 pairs (tout: toff[n] + 16 bytes) from a pack of targets: place[t] is target t's place in the
// pack's order, tdw[place] its first dword; pairStart null: column 0.  base: n long longs of scratch, left filled.
extern "C" int pairs_gather_cells_host(const uint32_t* pack, long long packDwords, const uint8_t* idToByte, const int* place,
                                       const long long* tdw, int n, const long long* toff, const int* pairTarget,
                                       const int* pairStart, long long* base, uint8_t* tout)
{
    uint16_t tab2[256];
    for (int c = 0; c < 256; ++c) tab2[c] = (uint16_t)(idToByte[c & 15] | idToByte[c >> 4] << 8);
    for (int p = 0; p < n; ++p) base[p] = cell_base(place, tdw, pairTarget[p], pairStart ? pairStart[p] : 0);
    TargetCellsSource ts{pack, packDwords, base};
    const long long total = toff[n];
    const long long blocks = (total + 16 + kBlockBytes - 1) / kBlockBytes;
    for (long long b = 0; b < blocks; ++b) {
        const int lo = find_pair_wave(toff, 0, n - 1, block_first(total, b));
        const int hi = find_pair_wave(toff, lo, block_far(lo, n), block_last(total, b));
        for (int t = 0; t < kBlockThreads; ++t) {
            const long long d0 = (b * kBlockThreads + t) * kRun;
            if (d0 >= total + 16) continue;
            Run r; r.w[0] = 0; r.w[1] = 0;
            if (d0 < total) r = target_run_cells(d0, total, find_pair(toff, lo, hi, d0), toff, ts, tab2);
            store_run_words(tout, d0, total, r.w[0], r.w[1]);
        }
    }
    return 0;
}

#if defined(PAIRS_GATHER_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <vector>

int main()
{
    unsigned seed = 2468;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    int failures = 0, pairs = 0;
    for (int sigma : {1, 4, 5, 16}) {
        uint8_t ids[16];
        for (int i = 0; i < 16; ++i) ids[i] = (uint8_t)(i < sigma ? (i % 3 == 2 ? 128 + 7 * i : 'A' + i) : 0);
        // the targets in the caller's order, packed in (length, index) order, each from a dword of its own; the heap block
        // is exactly the pack: the last target ends in its last dword
        const int lens[] = {33, 1, 400, 8, 2, 17, 7, 64, 9, 16, 15, 32, 31, 8, 400};
        const int nt = (int)(sizeof lens / sizeof lens[0]);
        std::vector<std::vector<uint8_t>> ts(nt);
        for (int t = 0; t < nt; ++t) {
            ts[t].resize(lens[t]);
            for (int j = 0; j < lens[t]; ++j) ts[t][j] = ids[sigma == 16 && j % 5 == 0 ? 15 : (int)(rnd() % sigma)];
        }
        std::vector<int> order(nt), place(nt);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] < lens[b]; });
        std::vector<long long> tdw(nt);
        long long ndw = 0;
        for (int i = 0; i < nt; ++i) { place[order[i]] = i; tdw[i] = ndw; ndw += (lens[order[i]] + 7) / 8; }
        uint32_t* pack = (uint32_t*)calloc((size_t)ndw, 4);
        for (int i = 0; i < nt; ++i)
            for (int j = 0; j < lens[order[i]]; ++j) {
                int code = 0;
                while (ids[code] != ts[order[i]][j]) ++code;
                pack[tdw[i] + (j >> 3)] |= (uint32_t)code << (4 * (j & 7));
            }
        // the pairs: every target whole, its last bases, every start phase with a few lengths
        std::vector<int> pt, ps, pl;
        for (int t = 0; t < nt; ++t) {
            pt.push_back(t); ps.push_back(0); pl.push_back(lens[t]);
            pt.push_back(t); ps.push_back(lens[t] - 1); pl.push_back(1);
            for (int s = 0; s < lens[t] && s < 9; ++s) { pt.push_back(t); ps.push_back(s); pl.push_back(1 + (int)(rnd() % (lens[t] - s))); }
        }
        const int n = (int)pt.size();
        std::vector<long long> toff(n + 1, 0), base(n);
        for (int p = 0; p < n; ++p) toff[p + 1] = toff[p] + pl[p];
        uint8_t* tout = (uint8_t*)malloc((size_t)toff[n] + 16);
        memset(tout, 0xEE, (size_t)toff[n] + 16);
        pairs_gather_cells_host(pack, ndw, ids, place.data(), tdw.data(), n, toff.data(), pt.data(), ps.data(), base.data(), tout);
        for (int p = 0; p < n; ++p)
            for (int j = 0; j < pl[p]; ++j)
                if (tout[toff[p] + j] != ts[pt[p]][ps[p] + j]) { ++failures; break; }
        for (int j = 0; j < 16; ++j)
            if (tout[toff[n] + j]) { ++failures; break; }
        // the whole-target form: no pairStart
        memset(tout, 0xEE, (size_t)toff[n] + 16);
        std::vector<long long> woff(nt + 1, 0);
        std::vector<int> all(nt);
        for (int t = 0; t < nt; ++t) { all[t] = nt - 1 - t; woff[t + 1] = woff[t] + lens[all[t]]; }
        uint8_t* wout = (uint8_t*)malloc((size_t)woff[nt] + 16);
        pairs_gather_cells_host(pack, ndw, ids, place.data(), tdw.data(), nt, woff.data(), all.data(), nullptr, base.data(), wout);
        for (int t = 0; t < nt; ++t)
            if (memcmp(wout + woff[t], ts[all[t]].data(), (size_t)lens[all[t]])) ++failures;
        pairs += n + nt;
        free(pack); free(tout); free(wout);
    }
    printf("pairs_gather_cells_host: %d pairs, %d failures\n", pairs, failures);
    return failures ? 1 : 0;
}
#endif
