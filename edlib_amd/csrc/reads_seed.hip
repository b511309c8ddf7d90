// reads_seed.hip -- exact k-mer seed filter of the reads-per-lane path: the first pass of an HW group of
// reads up to 256 bases against a shared target of at most four symbols, in place of the banded scan over every column.
//
// A read of m symbols is cut into p = k + 1 consecutive pieces (lengths floor(m / p) or one more).  An alignment with <= k
// edits leaves one piece without an edit (pigeonhole), so that piece occurs exactly in the target, and the alignment lies in
// the window [delta - k, delta + m - 1 + k] of the diagonal delta = P - o of that occurrence.  An HW scan restarted at the
// window's first column computes D' >= D for every column of the window, with equality wherever D <= k (the restart rule of
// DESIGN.md §1).  So: look every piece up exactly, merge the windows of a read, scan them with the whole read, and the least
// D' over the windows with the columns attaining it are the reads path's result whenever that least value is <= k.
// tests/seed_model.py is the same argument in numpy, checked against the textbook DP.
//
//   * the index: direct-address buckets on the first kSeedQ = 12 symbols of every target position (4^12 + 1 offsets,
//     T positions), built from the 2-bit packed target by a count kernel, rocPRIM's exclusive scan and a fill kernel;
//   * the seed + verify kernel: a lane per slot, a wave 64 consecutive slots (kernel A's layout).  The lane's Peq rows
//     (g.d_peq, [readBlock][4][NWD][64]) are its read: the 2-bit code of a query symbol is which row has its bit, a symbol
//     in no row (a byte the target lacks) makes its piece impossible.  Diagonals go into a sorted, duplicate-free list in
//     LDS; windows are merged and verified with the column of scan_reads_kernel, the target symbol of a lane's column
//     gathered from the packed target and its Eq row picked per lane from the four rows.
//   * hand-back: a read whose lookup is not cheap (a bucket of more than kSeedBucketCap positions, more than
//     kSeedMaxDiag distinct diagonals, a merged window longer than kSeedMaxWindow columns, a piece shorter than kSeedQ) is
//     listed; the host scans the list with the banded kernel over the whole target at the same threshold.
#include "reads_seed.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace edlib_amd {


// ------------------------------------------------------------------ the index

__global__ void __launch_bounds__(256)
seed_count_kernel(const u32* __restrict__ tpk, int npos, u32* __restrict__ cnt)
{
    const int P = blockIdx.x * blockDim.x + threadIdx.x;
    if (P >= npos) return;
    const u32 key = stream_bits(tpk[P >> 4], tpk[(P >> 4) + 1], (u32)P) & ((1u << (2 * kSeedQ)) - 1u);
    atomicAdd(&cnt[key], 1u);
}

// cnt counts down to zero again, so the next run's count starts from a zeroed table as well
__global__ void __launch_bounds__(256)
seed_fill_kernel(const u32* __restrict__ tpk, int npos, const u32* __restrict__ off, u32* __restrict__ cnt,
                 u32* __restrict__ pos)
{
    const int P = blockIdx.x * blockDim.x + threadIdx.x;
    if (P >= npos) return;
    const u32 key = stream_bits(tpk[P >> 4], tpk[(P >> 4) + 1], (u32)P) & ((1u << (2 * kSeedQ)) - 1u);
    pos[off[key] + atomicSub(&cnt[key], 1u) - 1u] = (u32)P;
}

hipError_t seed_index_scratch_bytes(size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const u32*)nullptr, (u32*)nullptr, 0u, kSeedBuckets + 1,
                                   rocprim::plus<u32>());
}

hipError_t launch_build_seed_index(const u32* tpk, int T, u32* cnt, u32* off, u32* pos, void* tmp, size_t tmpBytes,
                                   hipStream_t stream)
{
    const int npos = T - kSeedQ + 1;                      // positions with a whole key
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)(kSeedBuckets + 1) * sizeof(u32), stream);
    if (e != hipSuccess) return e;
    if (npos > 0) {
        hipLaunchKernelGGL(seed_count_kernel, dim3((npos + 255) / 256), dim3(256), 0, stream, tpk, npos, cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    size_t bytes = tmpBytes;
    e = rocprim::exclusive_scan(tmp, bytes, cnt, off, 0u, kSeedBuckets + 1, rocprim::plus<u32>(), stream);
    if (e != hipSuccess || npos <= 0) return e;
    hipLaunchKernelGGL(seed_fill_kernel, dim3((npos + 255) / 256), dim3(256), 0, stream, tpk, npos, off, cnt, pos);
    return hipGetLastError();
}


hipError_t launch_seed_verify(int nwords, const SeedArgs& a, hipStream_t stream)
{
    if (a.nslots == 0) return hipSuccess;
    const dim3 grid(a.nslots / 64), block(64);
    switch (nwords) {
#define CASE(N) case N: hipLaunchKernelGGL(seed_verify_kernel<N>, grid, block, 0, stream, a); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------ slot lists

namespace {
struct OpenSlot {
    const int *perm, *total, *qlen; int kcfg, kDone, mates;
    __device__ bool operator()(int s) const
    {
        if (perm[s] < 0 || total[s] > 0) return false;
        if (mates && total[s ^ 1] > 0) return false;      // both strands: the mate resolved at a threshold this slot missed
        const int m = qlen[s];
        return (kcfg < 0 ? m : min(m, kcfg)) > kDone;
    }
};
struct FlaggedSlot {
    const int *perm, *flags, *win;                        // win (both strands): strands.hpp's code of the pair s >> 1
    __device__ bool operator()(int s) const
    {
        if (flags[s] == 0 || perm[s] < 0) return false;
        return !win || (win[s >> 1] & 1) == (s & 1);      // a slot whose mate is reported never shows its list
    }
};
}  // namespace

hipError_t select_slots_scratch_bytes(int nslots, size_t* bytes)
{
    size_t a = 0, b = 0;
    hipError_t e = rocprim::select(nullptr, a, rocprim::counting_iterator<int>(0), (int*)nullptr, (int*)nullptr, (size_t)nslots,
                                   OpenSlot{});
    if (e != hipSuccess) return e;
    e = rocprim::select(nullptr, b, rocprim::counting_iterator<int>(0), (int*)nullptr, (int*)nullptr, (size_t)nslots,
                        FlaggedSlot{});
    *bytes = a > b ? a : b;
    return e;
}

hipError_t launch_select_open_slots(const int* perm, const int* total, const int* qlen, int kcfg, int kDone, int nslots,
                                    int* out, int* count, void* tmp, size_t tmpBytes, hipStream_t stream, bool mates)
{
    size_t bytes = tmpBytes;
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<int>(0), out, count, (size_t)nslots,
                           OpenSlot{perm, total, qlen, kcfg, kDone, mates ? 1 : 0}, stream);
}

hipError_t launch_select_flagged_slots(const int* perm, const int* flags, int nslots, int* out, int* count,
                                       void* tmp, size_t tmpBytes, hipStream_t stream, const int* win)
{
    size_t bytes = tmpBytes;
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<int>(0), out, count, (size_t)nslots,
                           FlaggedSlot{perm, flags, win}, stream);
}

__global__ void __launch_bounds__(256)
pick_slot_records_kernel(const int* __restrict__ slots, int n, const int* __restrict__ flags, const int* __restrict__ total,
                         int* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    out[3 * i] = s; out[3 * i + 1] = flags[s]; out[3 * i + 2] = total[s];
}

hipError_t launch_pick_slot_records(const int* slots, int n, const int* flags, const int* total, int* out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pick_slot_records_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, slots, n, flags, total, out);
    return hipGetLastError();
}

}  // namespace edlib_amd
