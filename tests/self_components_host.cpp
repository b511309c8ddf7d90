// self_components_host.cpp -- edlib_amd/csrc/self_components_core.hpp compiled for the HOST: the union-find of
// edlibAmdBatchSelfComponents on __atomic builtins, its edges split over std::threads the way the device splits them over
// lanes (thread t takes the edges t, t + T, t + 2 T ...), then the flatten by chasing.  A shared library for
// tests/test_self_components_model.py; with -DSELF_COMPONENTS_MAIN a program of its own that draws its graphs itself and
// checks every answer against a serial union-find (the sanitizer builds: address + undefined, and thread).
#include "../edlib_amd/csrc/self_components_core.hpp"

#include <thread>
#include <vector>

namespace sc = edlib_amd::self_components;

// work(e) for every e in [0, m), interleaved over `threads` threads
template <typename F>
static void split(long long m, int threads, F&& work)
{
    if (threads <= 1) {
        for (long long e = 0; e < m; ++e) work(e);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([=] { for (long long e = t; e < m; e += threads) work(e); });
    for (auto& x : th) x.join();
}

static void flatten(const std::vector<int>& parent, int n, int* label)
{
    for (int i = 0; i < n; ++i) label[i] = sc::uf_chase(parent.data(), i);
}

static std::vector<int> roots(int n)
{
    std::vector<int> parent(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) parent[i] = i;
    return parent;
}

extern "C" {

// edges (ei[e], ej[e]) in the order given
int self_components_host_edges(int n, const int* ei, const int* ej, long long m, int threads, int* label)
{
    std::vector<int> parent = roots(n);
    int* p = parent.data();
    split(m, threads, [=](long long e) { sc::uf_union(p, ei[e], ej[e]); });
    flatten(parent, n, label);
    return 0;
}

// the hit-list form: entry order[e] (order == nullptr: e) of a CSR list, its sorted keys (row << 32) | partner made here
int self_components_host_hits(int n, const long long* off, const int* partner, const int* ed, long long numHits, int level,
                              const long long* order, int threads, int* label)
{
    std::vector<int> parent = roots(n);
    int* p = parent.data();
    std::vector<unsigned long long> keys((size_t)numHits);
    for (int r = 0; r < n; ++r)
        for (long long e = off[r]; e < off[r + 1]; ++e)
            keys[(size_t)e] = ((unsigned long long)(uint32_t)r << 32) | (uint32_t)partner[e];
    const unsigned long long* skey = keys.data();
    split(numHits, threads, [=](long long e) { sc::hook_hit(p, skey, partner, ed, order ? order[e] : e, level); });
    flatten(parent, n, label);
    return 0;
}

// the dense form: every cell (i, j), i < j, of a condensed vector, row by row
int self_components_host_dense(int n, const int* cond, int level, int threads, int* label)
{
    std::vector<int> parent = roots(n);
    int* p = parent.data();
    const long long cells = (long long)n * (n - 1) / 2;
    std::vector<int> ri, rj;
    ri.reserve(cells > 0 ? cells : 0); rj.reserve(cells > 0 ? cells : 0);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) { ri.push_back(i); rj.push_back(j); }
    const int* pi = ri.data(); const int* pj = rj.data();
    split(cells > 0 ? cells : 0, threads, [=](long long c) { sc::hook_cell(p, cond, n, pi[c], pj[c], level); });
    flatten(parent, n, label);
    return 0;
}

}  // extern "C"

#ifdef SELF_COMPONENTS_MAIN
#include <algorithm>
#include <cstdio>
#include <random>

// the serial answer: union by minimum
static std::vector<int> serial(int n, const std::vector<int>& ei, const std::vector<int>& ej)
{
    std::vector<int> parent(n);
    for (int i = 0; i < n; ++i) parent[i] = i;
    auto find = [&](int x) { while (parent[x] != x) x = parent[x]; return x; };
    for (size_t e = 0; e < ei.size(); ++e) {
        const int a = find(ei[e]), b = find(ej[e]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    std::vector<int> label(n);
    for (int i = 0; i < n; ++i) label[i] = find(i);
    return label;
}

int main()
{
    std::mt19937 rng(12345);
    long long checks = 0, failures = 0;
    const int sizes[] = {1, 2, 3, 7, 64, 65, 150, 300};
    for (int n : sizes)
        for (int shape = 0; shape < 5; ++shape) {
            // a labelling of the vertices: the shapes below are drawn over a random order of the indices
            std::vector<int> name(n);
            for (int i = 0; i < n; ++i) name[i] = i;
            std::shuffle(name.begin(), name.end(), rng);
            std::vector<int> ei, ej;
            auto add = [&](int a, int b) { if (a != b) { ei.push_back(name[a]); ej.push_back(name[b]); } };
            if (shape == 0) for (int i = 0; i + 1 < n; ++i) add(i, i + 1);                       // a chain
            if (shape == 1) for (int i = 1; i < n; ++i) add(n - 1, i - 1);                       // a star
            if (shape == 2)                                                                      // cliques of 9
                for (int i = 0; i < n; ++i) for (int j = i + 1; j < n && j / 9 == i / 9; ++j) add(i, j);
            if (shape == 3) for (int i = 1; i < n; ++i) if (i % 11) add(i, (int)(rng() % i));    // a forest
            if (shape == 4) for (int e = 0; e < n; ++e) add((int)(rng() % n), (int)(rng() % n)); // sparse and random
            const size_t m0 = ei.size();
            for (size_t e = 0; e < m0; e += 3) { ei.push_back(ej[e]); ej.push_back(ei[e]); }     // duplicates, turned round
            const std::vector<int> want = serial(n, ei, ej);
            std::vector<size_t> order(ei.size());
            for (size_t e = 0; e < order.size(); ++e) order[e] = e;
            for (int round = 0; round < 3; ++round) {
                std::vector<int> si(ei.size()), sj(ej.size());
                for (size_t e = 0; e < order.size(); ++e) { si[e] = ei[order[e]]; sj[e] = ej[order[e]]; }
                for (int threads : {1, 2, 8}) {
                    std::vector<int> got(n, -1);
                    self_components_host_edges(n, si.data(), sj.data(), (long long)si.size(), threads, got.data());
                    ++checks;
                    if (got != want) { ++failures; printf("FAIL edges n=%d shape=%d round=%d threads=%d\n", n, shape, round, threads); }
                }
                std::shuffle(order.begin(), order.end(), rng);
            }
            // the same graph as a condensed vector and as its hit list, at the level that keeps the edges (distance 1)
            // beside pairs at 2 (above the level) and -1 (not reported)
            const long long cells = (long long)n * (n - 1) / 2;
            std::vector<int> cond((size_t)cells, -1);
            for (long long c = 0; c < cells; c += 5) cond[(size_t)c] = 2;
            for (size_t e = 0; e < ei.size(); ++e)
                cond[(size_t)sc::condensed_at(n, std::min(ei[e], ej[e]), std::max(ei[e], ej[e]))] = 1;
            std::vector<long long> off(n + 1, 0);
            std::vector<int> partner, ed;
            for (int i = 0; i < n; ++i) {
                for (int j = i + 1; j < n; ++j) {
                    const int d = cond[(size_t)sc::condensed_at(n, i, j)];
                    if (d >= 0) { partner.push_back(j); ed.push_back(d); }
                }
                off[i + 1] = (long long)partner.size();
            }
            for (int threads : {1, 8}) {
                std::vector<int> got(n, -1);
                self_components_host_dense(n, cond.data(), 1, threads, got.data());
                ++checks;
                if (got != want) { ++failures; printf("FAIL dense n=%d shape=%d threads=%d\n", n, shape, threads); }
                std::fill(got.begin(), got.end(), -1);
                self_components_host_hits(n, off.data(), partner.data(), ed.data(), (long long)partner.size(), 1, nullptr,
                                          threads, got.data());
                ++checks;
                if (got != want) { ++failures; printf("FAIL hits n=%d shape=%d threads=%d\n", n, shape, threads); }
            }
        }
    printf("%lld checks, %lld failures\n", checks, failures);
    return failures != 0;
}
#endif
