// neighbors_host.cpp -- the schedule of the neighbours selection (edlib_amd/csrc/neighbors_core.hpp) run on the host over
// arrays of 64, a "wave" whose lanes are array slots: the 21 sort stages, the reversed minimum and the six merge stages,
// the chunk loop with its skip, the write-out rule, and the index arithmetic of the accessors.  Checked against
// std::sort / std::partial_sort.  A program of its own (tests/test_neighbors_model.py builds it with
// -fsanitize=address,undefined and runs it as a child process); prints "<n> failures".
#include "../edlib_amd/csrc/neighbors_core.hpp"

#include <algorithm>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

namespace nb = edlib_amd::neighbors;
typedef nb::u64 u64;
typedef uint32_t u32;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
    std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Wave { u64 key[nb::kLanes]; u32 pay[nb::kLanes]; };

// one compare-exchange stage: every lane reads its partner's (key, payload) as they were in front of the stage
template <typename KeepsMin>
static void stage(Wave& w, int distance, KeepsMin keepsMin)
{
    const Wave before = w;
    for (int lane = 0; lane < nb::kLanes; ++lane) {
        const int p = nb::partner_lane(lane, distance);
        if (nb::takes_partner(keepsMin(lane), before.key[lane], before.key[p])) { w.key[lane] = before.key[p]; w.pay[lane] = before.pay[p]; }
    }
}

static void sort_chunk(Wave& c)
{
    for (int s = 0; s < nb::kSortStages; ++s) stage(c, nb::sort_distance(s), [s](int lane) { return nb::sort_keeps_min(s, lane); });
}

static void merge_chunk(Wave& list, const Wave& sorted)
{
    for (int lane = 0; lane < nb::kLanes; ++lane) {
        const int r = nb::reversed_lane(lane);
        if (sorted.key[r] < list.key[lane]) { list.key[lane] = sorted.key[r]; list.pay[lane] = sorted.pay[r]; }
    }
    for (int s = 0; s < nb::kMergeStages; ++s) stage(list, nb::merge_distance(s), [s](int lane) { return nb::merge_keeps_min(s, lane); });
}

struct Row { int count; std::vector<int> neighbor, distance; std::vector<u32> pay; long long merged; };

// the kernel's loop over a row of candidates (distance, index, payload): chunks of 64, the skip behind the K-th key
static Row select(const std::vector<int>& d, const std::vector<int>& index, int K, int level)
{
    Wave list;
    for (int l = 0; l < nb::kLanes; ++l) { list.key[l] = nb::kNoKey; list.pay[l] = 0; }
    u64 kth = nb::kNoKey;
    Row out{0, std::vector<int>(K, -1), std::vector<int>(K, -1), std::vector<u32>(K, 0), 0};
    const long long length = (long long)d.size();
    for (long long c0 = 0; c0 < length; c0 += nb::kLanes) {
        Wave chunk;
        bool any = false;
        for (int l = 0; l < nb::kLanes; ++l) {
            const long long c = c0 + l;
            chunk.key[l] = c < length ? nb::candidate_key(d[(size_t)c], index[(size_t)c], level) : nb::kNoKey;
            chunk.pay[l] = c < length ? (u32)c : 0;
            any = any || chunk.key[l] < kth;
        }
        if (!any) continue;
        ++out.merged;
        sort_chunk(chunk);
        for (int l = 1; l < nb::kLanes; ++l) CHECK(chunk.key[l - 1] <= chunk.key[l], "chunk not sorted at lane %d", l);
        merge_chunk(list, chunk);
        for (int l = 1; l < nb::kLanes; ++l) CHECK(list.key[l - 1] <= list.key[l], "list not sorted at lane %d", l);
        kth = list.key[K - 1];
    }
    int kept = 0;
    for (int l = 0; l < K; ++l) kept += list.key[l] != nb::kNoKey;
    out.count = nb::reported(K, kept);
    for (int l = 0; l < out.count; ++l) {
        out.neighbor[l] = nb::key_index(list.key[l]); out.distance[l] = nb::key_distance(list.key[l]); out.pay[l] = list.pay[l];
    }
    return out;
}

// the same row by std::partial_sort over the keys
static void check_row(const char* what, const std::vector<int>& d, const std::vector<int>& index, int K, int level,
                      long long wantMerged = -1)
{
    std::vector<std::pair<u64, u32>> keys;
    for (size_t c = 0; c < d.size(); ++c)
        if (nb::within(d[c], level)) keys.push_back({nb::make_key(d[c], index[c]), (u32)c});
    const size_t top = std::min(keys.size(), (size_t)K);
    std::partial_sort(keys.begin(), keys.begin() + top, keys.end());
    const Row got = select(d, index, K, level);
    CHECK(got.count == (int)top, "%s: K %d level %d: count %d, want %zu", what, K, level, got.count, top);
    for (int r = 0; r < K; ++r) {
        const bool have = r < (int)top;
        const int wn = have ? nb::key_index(keys[r].first) : -1, wd = have ? nb::key_distance(keys[r].first) : -1;
        CHECK(got.neighbor[r] == wn && got.distance[r] == wd, "%s: K %d level %d rank %d: (%d, %d), want (%d, %d)", what, K,
              level, r, got.neighbor[r], got.distance[r], wn, wd);
        if (have) CHECK(got.pay[r] == keys[r].second, "%s: K %d rank %d: payload %u, want %u", what, K, r, got.pay[r], keys[r].second);
    }
    if (wantMerged >= 0) CHECK(got.merged == wantMerged, "%s: K %d: %lld chunks merged, want %lld", what, K, got.merged, wantMerged);
}

static std::vector<int> iota(int n) { std::vector<int> v(n); for (int i = 0; i < n; ++i) v[i] = i; return v; }

int main()
{
    std::mt19937_64 rng(12345);
    const int Ks[] = {1, 2, 5, 63, 64};

    // the schedule itself: 21 stages with distances inside their runs, every lane paired once per stage, the two lanes of
    // a pair on opposite sides
    int stages = 0;
    for (int p = 1; p <= 6; ++p)
        for (int j = 1 << (p - 1); j >= 1; j >>= 1, ++stages) {
            CHECK(nb::sort_run(stages) == 1 << p && nb::sort_distance(stages) == j, "stage %d: run %d distance %d", stages,
                  nb::sort_run(stages), nb::sort_distance(stages));
            for (int lane = 0; lane < nb::kLanes; ++lane) {
                const int q = nb::partner_lane(lane, j);
                CHECK(q >= 0 && q < nb::kLanes && q != lane && nb::partner_lane(q, j) == lane, "stage %d lane %d", stages, lane);
                CHECK(nb::sort_keeps_min(stages, lane) != nb::sort_keeps_min(stages, q), "stage %d lane %d: one side", stages, lane);
            }
        }
    CHECK(stages == nb::kSortStages, "%d sort stages", stages);
    for (int s = 0; s < nb::kMergeStages; ++s)
        for (int lane = 0; lane < nb::kLanes; ++lane)
            CHECK(nb::merge_keeps_min(s, lane) != nb::merge_keeps_min(s, nb::partner_lane(lane, nb::merge_distance(s))), "merge %d", s);

    // random 64-key inputs, with -1 entries and heavy ties: the sort against std::sort, payloads riding along
    for (int round = 0; round < 200; ++round) {
        Wave w;
        std::vector<std::pair<u64, u32>> want;
        std::vector<int> perm = iota(64);
        std::shuffle(perm.begin(), perm.end(), rng);
        for (int l = 0; l < 64; ++l) {
            const int d = (int)(rng() % 5) - 1;
            w.key[l] = nb::candidate_key(d, perm[l], round % 3 == 0 ? 2 : -1);
            w.pay[l] = 1000u + (u32)perm[l];
            want.push_back({w.key[l], w.key[l] == nb::kNoKey ? 0u : w.pay[l]});
        }
        std::sort(want.begin(), want.end());
        sort_chunk(w);
        for (int l = 0; l < 64; ++l)
            CHECK(w.key[l] == want[l].first && (w.key[l] == nb::kNoKey || w.pay[l] == want[l].second), "random sort %d lane %d", round, l);
    }

    for (int K : Ks) {
        // all-equal distances: the index alone decides
        for (int n : {1, 63, 64, 65, 200}) {
            std::vector<int> idx = iota(n);
            std::shuffle(idx.begin(), idx.end(), rng);
            check_row("all equal", std::vector<int>(n, 3), idx, K, -1);
        }
        // strictly descending keys: every chunk replaces the whole list (all of them are merged)
        {
            const int n = 640;
            std::vector<int> d(n);
            for (int c = 0; c < n; ++c) d[c] = n - c;
            check_row("descending", d, iota(n), K, -1, n / 64);
        }
        // strictly ascending keys: nothing enters after the first chunk (one merge)
        {
            const int n = 640;
            std::vector<int> d(n);
            for (int c = 0; c < n; ++c) d[c] = c;
            check_row("ascending", d, iota(n), K, -1, 1);
        }
        // streams of 1, 63, 64, 65, 128 and 129 candidates against std::partial_sort, at every level
        for (int n : {0, 1, 63, 64, 65, 128, 129, 1000})
            for (int level : {-1, 0, 1, 3})
                for (int round = 0; round < 8; ++round) {
                    std::vector<int> d(n), idx = iota(n);
                    for (int& x : d) x = (int)(rng() % 7) - 1;
                    std::shuffle(idx.begin(), idx.end(), rng);
                    check_row("stream", d, idx, K, level);
                }
        // no candidate at all within the level
        check_row("none", std::vector<int>(100, 5), iota(100), K, 2, 0);
    }

    // the order in which a row's entries are met does not matter: a shuffled row gives the same row
    for (int round = 0; round < 50; ++round) {
        const int n = 300;
        std::vector<int> d(n), idx = iota(n), order = iota(n);
        for (int& x : d) x = (int)(rng() % 4);
        const Row a = select(d, idx, 64, -1);
        std::shuffle(order.begin(), order.end(), rng);
        std::vector<int> d2(n), idx2(n);
        for (int c = 0; c < n; ++c) { d2[c] = d[order[c]]; idx2[c] = idx[order[c]]; }
        const Row b = select(d2, idx2, 64, -1);
        CHECK(a.count == b.count && a.neighbor == b.neighbor && a.distance == b.distance, "order dependence in round %d", round);
    }

    // the condensed index arithmetic: the cells in scipy's pdist order, either order of the pair; the matrix and the CSR
    for (int n : {2, 3, 64, 65}) {
        long long at = 0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j, ++at) {
                CHECK(nb::condensed_at(n, i, j) == at && nb::condensed_at(n, j, i) == at, "condensed n %d (%d, %d)", n, i, j);
            }
        CHECK(at == (long long)n * (n - 1) / 2, "condensed size n %d", n);
    }
    CHECK(nb::matrix_at(96, 1000000, 95) == 96000095LL, "matrix_at");
    CHECK(nb::matrix_at(65536, 65535, 65535) == 4294967295LL, "matrix_at past 2^31");
    CHECK(nb::condensed_at(200000, 199998, 199999) == 200000LL * 199999 / 2 - 1, "condensed_at past 2^31");
    CHECK(nb::csr_at(1LL << 33, 5) == (1LL << 33) + 5, "csr_at");
    CHECK(nb::chunks_of(0) == 0 && nb::chunks_of(1) == 1 && nb::chunks_of(64) == 1 && nb::chunks_of(65) == 2, "chunks_of");
    CHECK(nb::make_key(3, 7) == ((3ull << 32) | 7) && nb::candidate_key(-1, 7, -1) == nb::kNoKey &&
          nb::candidate_key(3, 7, 2) == nb::kNoKey && nb::candidate_key(2, 7, 2) == ((2ull << 32) | 7), "keys");

    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
