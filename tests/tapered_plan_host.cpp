// The segment planner of the reads path (edlib_amd/csrc/segment_plan.hpp) compiled for the host alone, for
// tests/test_tapered_plan.py.
#include "../edlib_amd/csrc/segment_plan.hpp"

using namespace edlib_amd;

extern "C" {

// the uniform plan of a HW launch: out = {S, segLen, warm}
void plan_uniform_host(int nlanes, int T, int warmFull, long long wantWaves, int minSegCols, int* out)
{
    plan_segments_uniform(nlanes, T, true, warmFull, wantWaves, minSegCols, out[0], out[1], out[2]);
}

// the tapered table: returns the number of segments, writes at most `room` of them as start, cols pairs
int plan_tapered_host(int T, int gridX, int resident, int warm, int Lmax, int* out, int room)
{
    const std::vector<Segment> t = plan_segments_tapered(T, gridX, resident, warm, Lmax);
    for (size_t i = 0; i < t.size() && (int)i < room; ++i) { out[2 * i] = t[i].start; out[2 * i + 1] = t[i].cols; }
    return (int)t.size();
}

}
