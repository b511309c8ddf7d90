// cross_kernels_self_groups.hip -- the grouped self instantiations of the cross scan (cross_scan.hpp, SELF and GROUPS: NW,
// hit list, one strand, 1..8 words, 4 / 8 / 16 symbols: 24 kernels) in a translation unit of their own (DESIGN.md §4h
// "Grouped self batches").
#include "cross_scan.hpp"

namespace edlib_amd {

// the grouped self ladder (hit list, one strand): one block per work item
template <int NWD>
static hipError_t launch_scan_self_groups_w(int syms, const CrossScanArgs& a, hipStream_t stream)
{
    const dim3 grid((unsigned)a.numItems);
    if (syms == 4) hipLaunchKernelGGL((scan_cross_kernel<NWD, 4, 0, true, false, true, true>), grid, dim3(64), 0, stream, a);
    else if (syms == 8) hipLaunchKernelGGL((scan_cross_kernel<NWD, 8, 0, true, false, true, true>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scan_cross_kernel<NWD, 16, 0, true, false, true, true>), grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

static hipError_t launch_scan_self_groups_h(int nwords, int syms, const CrossScanArgs& a, hipStream_t stream)
{
    switch (nwords) {
    case 1: return launch_scan_self_groups_w<1>(syms, a, stream);
    case 2: return launch_scan_self_groups_w<2>(syms, a, stream);
    case 3: return launch_scan_self_groups_w<3>(syms, a, stream);
    case 4: return launch_scan_self_groups_w<4>(syms, a, stream);
    case 5: return launch_scan_self_groups_w<5>(syms, a, stream);
    case 6: return launch_scan_self_groups_w<6>(syms, a, stream);
    case 7: return launch_scan_self_groups_w<7>(syms, a, stream);
    case 8: return launch_scan_self_groups_w<8>(syms, a, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_cross_self_groups(int nwords, int syms, const CrossScanArgs& a, hipStream_t stream)
{
    if (a.numItems == 0) return hipSuccess;
    const int st = cross_scan_args_state(syms, 0, true, a);
    if (st) return st > 0 ? hipSuccess : hipErrorInvalidValue;
    if (a.numItems < 0 || !a.items || !a.qrank || !a.qend) return hipErrorInvalidValue;
    return launch_scan_self_groups_h(nwords, syms, a, stream);
}

}  // namespace edlib_amd
