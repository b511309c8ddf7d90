// self_groups_layout.cpp -- the host layout of a grouped self batch (edlib_amd/csrc/self_groups_layout.hpp) over a label /
// length set read from a file, as counters: what tools/bench_self_groups.py records beside its timings.
//   self_groups_layout <file> <k>      file: int32 n, then n int32 labels, then n int32 lengths (1..256 bases each)
// Prints one JSON line: sequences, word groups with their tile widths, items, trips, wanted pairs, live-lane share
// (wanted pairs / (64 * trips)), word_steps, and the milliseconds the layout took.
#include "../edlib_amd/csrc/self_groups_layout.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <file> <k>\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    int n = 0;
    if (!f || std::fread(&n, sizeof n, 1, f) != 1 || n < 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<int> group((size_t)n), len((size_t)n), seqs((size_t)n);
    if (std::fread(group.data(), sizeof(int), (size_t)n, f) != (size_t)n || std::fread(len.data(), sizeof(int), (size_t)n, f) != (size_t)n) {
        std::fprintf(stderr, "%s is short\n", argv[1]);
        return 2;
    }
    std::fclose(f);
    for (int i = 0; i < n; ++i) {
        if (len[i] < 1 || len[i] > 256) { std::fprintf(stderr, "length %d of sequence %d is outside 1..256\n", len[i], i); return 2; }
        seqs[i] = i;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const edlib_amd::SelfGroupsLayout L = edlib_amd::self_groups_layout(std::move(seqs), [&](int i) { return group[i]; },
                                                                        [&](int i) { return len[i]; }, std::atoi(argv[2]), 8);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    long long items = 0;
    std::printf("{\"sequences\": %d, \"word_groups\": [", n);
    for (size_t g = 0; g < L.wordGroups.size(); ++g) {
        const edlib_amd::SelfGroupsWordGroup& w = L.wordGroups[g];
        items += (long long)w.items.size() / 3;
        std::printf("%s{\"words\": %d, \"qt\": %d, \"tiles\": %d, \"items\": %zu, \"trips\": %lld}", g ? ", " : "", w.words, w.qt,
                    w.tiles, w.items.size() / 3, w.trips);
    }
    std::printf("], \"items\": %lld, \"trips\": %lld, \"wanted_pairs\": %lld, \"live_lane_share\": %.4f, \"word_steps\": %lld, "
                "\"layout_ms\": %.1f}\n", items, L.trips, L.wanted, L.trips ? (double)L.wanted / (64.0 * (double)L.trips) : 0.0,
                L.wordSteps, ms);
    return 0;
}
