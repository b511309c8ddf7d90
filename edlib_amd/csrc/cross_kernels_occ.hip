// cross_kernels_occ.hip -- the occurrence instantiations of the lane-per-cell scan (cross_scan.hpp, scan_cross_occ_kernel;
// DESIGN.md §4h "Occurrence batches"): HW only, word counts 1..8, S = 4 / 8 / 16.  A translation unit of its own, as the
// other instantiation halves, for the parallel build.
#include "cross_scan.hpp"

namespace edlib_amd {

hipError_t launch_scan_cross_occ(int nwords, int syms, const CrossScanArgs& a, int ysplit, hipStream_t stream)
{
    const int st = cross_scan_args_state(syms, 2, true, a);
    if (st) return st > 0 ? hipSuccess : hipErrorInvalidValue;
    if (a.kcfg < 0) return hipErrorInvalidValue;
    switch (nwords) {
    case 1: return launch_scan_cross_occ_w<1>(syms, a, ysplit, stream);
    case 2: return launch_scan_cross_occ_w<2>(syms, a, ysplit, stream);
    case 3: return launch_scan_cross_occ_w<3>(syms, a, ysplit, stream);
    case 4: return launch_scan_cross_occ_w<4>(syms, a, ysplit, stream);
    case 5: return launch_scan_cross_occ_w<5>(syms, a, ysplit, stream);
    case 6: return launch_scan_cross_occ_w<6>(syms, a, ysplit, stream);
    case 7: return launch_scan_cross_occ_w<7>(syms, a, ysplit, stream);
    case 8: return launch_scan_cross_occ_w<8>(syms, a, ysplit, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace edlib_amd
