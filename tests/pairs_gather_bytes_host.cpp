// pairs_gather_bytes_host.cpp -- TEST INFRASTRUCTURE: the device code that gathers a pair batch's target pool from a read
// batch's raw target (edlib_amd/csrc/pairs_gather_core.hpp: bytes16, target_run_bytes) compiled for the host, the
// destination runs walked one by one in the kernel's order: block, thread, the block's pair range, the thread's pair, the
// run, the store.  Built by tests/test_pairs_gather_bytes_model.py with g++ into build/libpairs_gather_bytes_host.so; with
// -DPAIRS_GATHER_BYTES_MAIN it is a program of its own that gathers a grid from exactly sized heap blocks and compares it
// with byte-wise slicing (the sanitizer build).  Never linked into the product.
#include "../edlib_amd/csrc/pairs_gather_core.hpp"

#include <string.h>

using namespace edlib_amd::pairs_gather;

// the kernel's wave search, the ballot counted lane by lane
static int find_pair_wave(const long long* off, int lo, int hi, long long pos)
{
    while (lo < hi) narrow(lo, hi, count_probes(off, lo, hi, pos));
    return lo;
}

// the kernel's store: 16 bytes where the pool (total + 16 bytes) has them, its last bytes otherwise
static void store_run(uint8_t* pool, long long d0, long long total, const Run& r)
{
    const long long left = total + 16 - d0;
    uint8_t b[kRun];
    for (int j = 0; j < kRun; ++j) b[j] = (uint8_t)(r.w[j >> 3] >> (8 * (j & 7)));
    memcpy(pool + d0, b, left >= kRun ? (size_t)kRun : (size_t)left);
}

// sixteen bytes from byte position s of a pool of ndw dwords
extern "C" void pairs_gather_bytes16(const uint32_t* pool, long long ndw, long long s, uint8_t* out)
{
    const Run r = bytes16(pool, ndw, s);
    for (int j = 0; j < kRun; ++j) out[j] = (uint8_t)(r.w[j >> 3] >> (8 * (j & 7)));
}

// The target pool of n >= 1 pairs (tout: toff[n] + 16 bytes) from the target as ndw dwords.  Returns 0.
extern "C" int pairs_gather_bytes_host(const uint32_t* tbytes, long long ndw, int n, const long long* toff,
                                       const int* pairStart, uint8_t* tout)
{
    TargetBytesSource ts{tbytes, ndw, pairStart};
    const long long total = toff[n];
    const long long blocks = (total + 16 + kBlockBytes - 1) / kBlockBytes;
    for (long long b = 0; b < blocks; ++b)
        for (int t = 0; t < kBlockThreads; ++t) {
            const long long d0 = (b * kBlockThreads + t) * kRun;
            if (d0 >= total + 16) continue;
            Run r; r.w[0] = 0; r.w[1] = 0;
            if (d0 < total) {
                const int lo = find_pair_wave(toff, 0, n - 1, block_first(total, b));
                const int hi = find_pair_wave(toff, lo, block_far(lo, n), block_last(total, b));
                r = target_run_bytes(d0, total, find_pair(toff, lo, hi, d0), toff, ts);
            }
            store_run(tout, d0, total, r);
        }
    return 0;
}

#if defined(PAIRS_GATHER_BYTES_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main()
{
    unsigned seed = 2468;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    // a target of 1,031 bytes over 40 distinct values, some >= 128, in a block of exactly the dwords the kernel may read:
    // (T + 16) / 4 of them, as a read batch allocates its target pool
    const int T = 1031;
    uint8_t alphabet[40];
    for (int i = 0; i < 40; ++i) alphabet[i] = (uint8_t)(i % 3 == 2 ? 130 + 3 * i : 40 + 2 * i);
    const long long ndw = (T + 16) / 4;
    uint32_t* pool = (uint32_t*)calloc((size_t)ndw, 4);
    uint8_t* target = (uint8_t*)pool;
    for (int j = 0; j < T; ++j) target[j] = alphabet[rnd() % 40];
    int failures = 0;

    // bytes16 at every position, the pool's end included: bytes behind the block are zero
    for (long long s = 0; s < 4 * ndw; ++s) {
        Run r = bytes16(pool, ndw, s);
        for (int j = 0; j < kRun; ++j) {
            const uint8_t want = s + j < 4 * ndw ? target[s + j] : 0;
            if ((uint8_t)(r.w[j >> 3] >> (8 * (j & 7))) != want) { ++failures; break; }
        }
    }

    // the pairs: every window length x every source byte phase x every destination phase (a filler pair in front moves
    // the pool to it), then windows at column 0 and up to the last column
    const int wl[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 400};
    std::vector<int> ps, pl;
    long long total = 0;
    auto add = [&](int s, int L) { ps.push_back(s); pl.push_back(L); total += L; };
    for (int L : wl)
        for (int sp = 0; sp < 4; ++sp)
            for (int dp = 0; dp < 16; ++dp) {
                const int fill = (int)(((dp - total) % 16 + 16) % 16);
                if (fill) add((int)(rnd() % (T - 16)), fill);
                add(4 * (int)(rnd() % ((T - L) / 4 + 1 - (sp ? 1 : 0))) + sp, L);
            }
    for (int L : wl) { add(0, L); add(T - L, L); }
    add(0, T);
    const int n = (int)ps.size();
    std::vector<long long> toff(n + 1, 0);
    for (int p = 0; p < n; ++p) {
        if (ps[p] < 0 || ps[p] + pl[p] > T) { printf("bad grid at %d\n", p); return 2; }
        toff[p + 1] = toff[p] + pl[p];
    }
    uint8_t* tout = (uint8_t*)malloc((size_t)toff[n] + 16);
    memset(tout, 0xEE, (size_t)toff[n] + 16);
    pairs_gather_bytes_host(pool, ndw, n, toff.data(), ps.data(), tout);
    for (int p = 0; p < n; ++p)
        for (int j = 0; j < pl[p]; ++j)
            if (tout[toff[p] + j] != target[ps[p] + j]) { ++failures; break; }
    for (int j = 0; j < 16; ++j)
        if (tout[toff[n] + j]) { ++failures; break; }
    free(pool); free(tout);
    printf("pairs_gather_bytes_host: %d pairs, %d failures\n", n, failures);
    return failures ? 1 : 0;
}
#endif
