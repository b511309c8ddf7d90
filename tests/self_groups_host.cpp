// self_groups_host.cpp -- the host layout of a grouped self batch (edlib_amd/csrc/self_groups_layout.hpp) run without a
// device: the order, ranks, ends, word groups, tiles and work items, then every (item, trip, lane) through the lane
// predicate the kernel shares with it.  Over random label / length sets and planted cases it checks that every wanted
// pair (same group, both 1..256 bases, lengths within k) is live exactly once, that no other lane is live inside the
// length window (a live lane outside it is a same-group pair the kernel answers -1 without a column, as an ungrouped self
// batch's does), that every trip of every item lies inside the range of one of its tile's runs, and that wordSteps is the
// sum over the live lanes.  A program of its own (tests/test_self_groups_model.py builds it with
// -fsanitize=address,undefined and runs it as a child process); prints "<n> failures".
#include "../edlib_amd/csrc/self_groups_layout.hpp"

#include <cstdio>
#include <random>
#include <string>

using namespace edlib_amd;
typedef unsigned long long u64;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
    std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int kMaxWords = 8;

struct Case { std::string name; std::vector<int> group, len; int k; };
struct Seen { long long items = 0, trips = 0, live = 0, outside = 0, wordSteps = 0, maxItemsOfATile = 0; size_t wordGroups = 0; };

static Seen check(const Case& c)
{
    Seen seen;
    const char* nm = c.name.c_str();
    const int n = (int)c.len.size();
    std::vector<int> seqs;
    for (int i = 0; i < n; ++i)
        if (c.len[i] >= 1 && c.len[i] <= 32 * kMaxWords) seqs.push_back(i);         // the kernel's envelope
    const SelfGroupsLayout L = self_groups_layout(seqs, [&](int i) { return c.group[i]; }, [&](int i) { return c.len[i]; },
                                                  c.k, kMaxWords, true);
    const int ns = (int)L.order.size();
    CHECK(ns == (int)seqs.size(), "%s: order holds %d of %zu", nm, ns, seqs.size());
    // the order (group, length, index), the lengths and the ends
    for (int r = 0; r < ns; ++r) {
        const int i = L.order[r];
        CHECK(L.tlen[r] == c.len[i], "%s: tlen[%d]", nm, r);
        if (r + 1 < ns) {
            const int j = L.order[r + 1];
            const bool asc = c.group[i] != c.group[j] ? c.group[i] < c.group[j] : (c.len[i] != c.len[j] ? c.len[i] < c.len[j] : i < j);
            CHECK(asc, "%s: ranks %d and %d are out of order", nm, r, r + 1);
            CHECK((L.end[r] == r + 1) == (c.group[i] != c.group[j]), "%s: end[%d] = %d", nm, r, L.end[r]);
            CHECK(c.group[i] != c.group[j] || L.end[r] == L.end[r + 1], "%s: end[%d] != end[%d] inside a group", nm, r, r + 1);
        } else CHECK(L.end[r] == ns, "%s: the last end is %d", nm, L.end[r]);
    }
    // the wanted pairs, by rank
    std::vector<u64> want, got;
    long long wantSteps = 0;
    for (int a = 0; a < ns; ++a)
        for (int b = a + 1; b < L.end[a] && L.tlen[b] - L.tlen[a] <= c.k; ++b) {
            want.push_back(((u64)a << 32) | (u64)b);
            wantSteps += (long long)((L.tlen[a] + 31) / 32) * L.tlen[b];
        }
    std::vector<char> isQuery(ns, 0);
    int lastWords = 0;
    for (const SelfGroupsWordGroup& g : L.wordGroups) {
        CHECK(g.words > lastWords && g.words <= kMaxWords, "%s: word groups ascend (%d after %d)", nm, g.words, lastWords);
        lastWords = g.words;
        const int qt = g.qt, tpt = qt ? 64 / qt : 0;
        CHECK(qt >= 1 && qt <= 64 && 64 % qt == 0, "%s: qt %d", nm, qt);
        if (qt < 1 || 64 % qt) continue;
        const size_t slots = (size_t)g.tiles * qt;
        CHECK(g.perm.size() == slots && g.rank.size() == slots && g.end.size() == slots, "%s: slot arrays", nm);
        CHECK(!g.items.empty() && g.items.size() % 3 == 0, "%s: a word group without items is kept", nm);
        // slot s holds the s-th rank of this word count, ascending; whole tiles, padding -1 behind
        int s = 0;
        for (int r = 0; r < ns; ++r)
            if ((L.tlen[r] + 31) / 32 == g.words) {
                CHECK((size_t)s < slots && g.rank[s] == r && g.perm[s] == L.order[r] && g.end[s] == L.end[r], "%s: slot %d of words %d", nm, s, g.words);
                isQuery[r] = 1;
                ++s;
            }
        CHECK(g.tiles == (s + qt - 1) / qt, "%s: tiles", nm);
        for (size_t p = (size_t)s; p < slots; ++p) CHECK(g.perm[p] == -1 && g.rank[p] == -1 && g.end[p] == -1, "%s: padding slot %zu", nm, p);
        // the runs by tile
        std::vector<size_t> runOff((size_t)g.tiles + 1, 0);
        for (const SelfGroupsRange& r : g.runs) { CHECK(r.tile >= 0 && r.tile < g.tiles && r.first <= r.last, "%s: run", nm); ++runOff[(size_t)r.tile + 1]; }
        for (int t = 0; t < g.tiles; ++t) runOff[t + 1] += runOff[t];
        for (size_t i = 1; i < g.runs.size(); ++i) CHECK(g.runs[i - 1].tile <= g.runs[i].tile, "%s: runs by tile", nm);
        long long groupSteps = 0, groupTrips = 0;
        std::vector<long long> itemsOfTile(g.tiles, 0);
        for (size_t it = 0; it + 2 < g.items.size(); it += 3) {
            const int tile = g.items[it], first = g.items[it + 1], trips = g.items[it + 2];
            CHECK(tile >= 0 && tile < g.tiles && first >= 0 && trips > 0, "%s: item %zu (%d, %d, %d)", nm, it / 3, tile, first, trips);
            if (tile < 0 || tile >= g.tiles) continue;
            CHECK((long long)(first + trips - 1) * tpt < ns, "%s: item %zu ends past the ranks", nm, it / 3);
            ++seen.items; ++itemsOfTile[tile];
            groupTrips += trips;
            for (int tt = first; tt < first + trips; ++tt) {
                bool inside = false;
                for (size_t r = runOff[tile]; r < runOff[tile + 1] && !inside; ++r) inside = g.runs[r].first <= tt && tt <= g.runs[r].last;
                CHECK(inside, "%s: trip %d of tile %d (words %d) is in no run's range", nm, tt, tile, g.words);
                for (int lane = 0; lane < 64; ++lane) {
                    int qi = -1, ts = -1;
                    const int slot = tile * qt + (lane & (qt - 1));
                    const bool live = self_groups_lane(qt, lane, tt, g.rank[slot], g.end[slot], ns, qi, ts);
                    CHECK(qi == (lane & (qt - 1)) && ts == tt * tpt + lane / qt, "%s: lane arithmetic", nm);
                    if (!live) continue;
                    const int rank = g.rank[slot];
                    CHECK(rank >= 0 && ts > rank && ts < ns, "%s: live lane of rank %d on %d", nm, rank, ts);
                    if (rank < 0 || ts >= ns) continue;
                    CHECK(L.end[ts] == L.end[rank], "%s: ranks %d and %d of different groups are live", nm, rank, ts);
                    if (L.tlen[ts] - L.tlen[rank] > c.k) { ++seen.outside; continue; }
                    got.push_back(((u64)rank << 32) | (u64)ts);
                    groupSteps += (long long)g.words * L.tlen[ts];
                }
            }
        }
        CHECK(groupSteps == g.wordSteps, "%s: words %d wordSteps %lld, live lanes %lld", nm, g.words, g.wordSteps, groupSteps);
        CHECK(groupTrips == g.trips, "%s: words %d trips", nm, g.words);
        seen.wordSteps += groupSteps; seen.trips += groupTrips;
        for (long long x : itemsOfTile) seen.maxItemsOfATile = std::max(seen.maxItemsOfATile, x);
    }
    // a row with a partner has a slot (a word group without any is dropped whole)
    for (u64 w : want) CHECK(isQuery[(size_t)(w >> 32)], "%s: rank %llu has a partner but no slot", nm, w >> 32);
    std::sort(got.begin(), got.end());
    for (size_t i = 1; i < got.size(); ++i) CHECK(got[i] != got[i - 1], "%s: pair (%llu, %llu) is live twice", nm, got[i] >> 32, got[i] & 0xffffffffull);
    CHECK(got == want, "%s: %zu live pairs inside the window, %zu wanted", nm, got.size(), want.size());
    CHECK(L.wordSteps == wantSteps && seen.wordSteps == wantSteps, "%s: wordSteps %lld, wanted %lld", nm, L.wordSteps, wantSteps);
    CHECK(L.wanted == (long long)want.size() && L.trips == seen.trips, "%s: wanted / trips counters", nm);
    seen.live = (long long)got.size();
    seen.wordGroups = L.wordGroups.size();
    std::printf("case %s n=%d k=%d word_groups=%zu items=%lld trips=%lld live=%lld outside=%lld word_steps=%lld\n", nm, n, c.k,
                seen.wordGroups, seen.items, seen.trips, seen.live, seen.outside, L.wordSteps);
    return seen;
}

// labels whose groups have the given sizes, interleaved: member x of every group in turn, then scattered by a stride
static std::vector<int> interleaved(const std::vector<int>& sizes, const std::vector<int>& label)
{
    std::vector<int> out;
    for (int x = 0;; ++x) {
        bool any = false;
        for (size_t g = 0; g < sizes.size(); ++g)
            if (x < sizes[g]) { out.push_back(label[g]); any = true; }
        if (!any) break;
    }
    return out;
}

int main()
{
    std::mt19937 rng(12345);
    auto uniform = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };

    // random sets: few and many labels (negative ones too), lengths in and out of the envelope, k 0..5
    for (int round = 0; round < 60; ++round) {
        Case c;
        c.name = "random" + std::to_string(round);
        const int n = uniform(0, 400), labels = round % 3 == 0 ? 3 : (round % 3 == 1 ? 40 : 400);
        const int lo = round % 4 == 0 ? 0 : 20, hi = round % 4 == 0 ? 300 : (round % 4 == 1 ? 40 : (round % 4 == 2 ? 70 : 24));
        c.k = uniform(0, 5);
        for (int i = 0; i < n; ++i) { c.group.push_back(uniform(-labels / 2, labels / 2) * 1000003); c.len.push_back(uniform(lo, hi)); }
        check(c);
    }

    // group sizes 1, 2, 3, 7, 8, 9, 63, 64, 65 with interleaved labels; lengths 20..40, so one and two words inside a group
    for (int k : {0, 2}) {
        Case c;
        c.name = "sizes_k" + std::to_string(k);
        c.k = k;
        c.group = interleaved({1, 2, 3, 7, 8, 9, 63, 64, 65}, {5, -7, 0, 2147483647, -2147483647 - 1, 11, -1, 3, 1});
        for (size_t i = 0; i < c.group.size(); ++i) c.len.push_back(uniform(20, 40));
        const Seen s = check(c);
        CHECK(s.wordGroups == 2, "sizes: one- and two-word groups expected, got %zu", s.wordGroups);
    }
    {   // one group of 1,500 among singletons: the chunk rule cuts its tiles' ranges
        Case c;
        c.name = "big_group";
        c.k = 2;
        for (int i = 0; i < 2000; ++i) { c.group.push_back(i % 4 == 3 ? 100 + i : 7); c.len.push_back(uniform(28, 32)); }
        const Seen s = check(c);
        CHECK(s.maxItemsOfATile >= 2, "big group: no tile's range was cut (%lld items)", s.items);
    }
    {   // three 200-base sequences, each with a 201-base partner in its group, scattered through 300 short ones in ten groups:
        // the seven-word group's one tile spans distant ranks, and ranges that neither overlap nor touch stay apart
        Case c;
        c.name = "scattered";
        c.k = 2;
        for (int i = 0; i < 300; ++i) { c.group.push_back(i % 10); c.len.push_back(uniform(20, 40)); }
        for (int g : {0, 4, 9}) {
            const size_t at = (size_t)uniform(0, (int)c.group.size());
            c.group.insert(c.group.begin() + at, g); c.len.insert(c.len.begin() + at, 200);
            c.group.push_back(g); c.len.push_back(201);
        }
        const Seen s = check(c);
        CHECK(s.wordGroups == 3, "scattered: one-, two- and seven-word groups expected, got %zu", s.wordGroups);
        CHECK(s.maxItemsOfATile >= 2, "scattered: the distant ranges of a tile were merged");
    }
    {   // all singletons: no item
        Case c;
        c.name = "singletons";
        c.k = 3;
        for (int i = 0; i < 500; ++i) { c.group.push_back(-250 + i); c.len.push_back(uniform(20, 40)); }
        const Seen s = check(c);
        CHECK(s.wordGroups == 0 && s.items == 0 && s.wordSteps == 0, "singletons: %lld items", s.items);
    }
    {   // 200,000 groups of 3 x 12 bases, labels scattered (the shape of the GPU test): more work items than a grid's y or z holds
        Case c;
        c.name = "small_groups";
        c.k = 1;
        for (int i = 0; i < 600000; ++i) { c.group.push_back((int)(((long long)i * 7919) % 200000) - 7); c.len.push_back(12); }
        const Seen s = check(c);
        CHECK(s.items > 65535 && s.live == 600000, "small groups: %lld items, %lld live", s.items, s.live);
    }
    for (int k : {0, 3}) {   // one group only: the pairs of an ungrouped self batch (the test holds word_steps against its formula)
        Case c;
        c.name = "one_group_k" + std::to_string(k);
        c.k = k;
        for (int i = 0; i < 700; ++i) { c.group.push_back(-3); c.len.push_back(20 + (i * 7) % 50); }
        check(c);
    }
    {   // the predicate on padding and at the ends
        int qi, ts;
        CHECK(!self_groups_lane(64, 5, 0, -1, -1, 100, qi, ts), "a padding slot is live");
        CHECK(!self_groups_lane(1, 63, 1, 10, 200, 100, qi, ts) && ts == 127, "a rank past numSorted is live");
        CHECK(self_groups_lane(8, 17, 2, 10, 19, 100, qi, ts) && qi == 1 && ts == 18, "lane 17 of qt 8 on tile 2");
        CHECK(!self_groups_lane(8, 25, 2, 10, 19, 100, qi, ts) && ts == 19, "the group's end is live");
        CHECK(!self_groups_lane(8, 1, 1, 9, 19, 100, qi, ts) && ts == 8, "a rank below the query's is live");
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
