// cross_kernels_strands.hip -- the both-strand instantiations of the cross scan (cross_scan.hpp, STRANDS = true): a
// translation unit of their own, as many kernels again as cross_kernels.hip compiles.
#include "cross_scan.hpp"

namespace edlib_amd {

hipError_t launch_scan_cross_strands(int nwords, int syms, int mode, bool hits, const CrossScanArgs& a, int ysplit,
                                     hipStream_t stream)
{
    const int st = cross_scan_args_state(syms, mode, hits, a);
    if (st) return st > 0 ? hipSuccess : hipErrorInvalidValue;
    // mates are neighbouring lanes: an even tile width, and somewhere to put the strand bytes
    if ((a.qt & 1) || !a.strand) return hipErrorInvalidValue;
    return hits ? launch_scan_cross_h<true, true>(nwords, syms, mode, a, ysplit, stream)
                : launch_scan_cross_h<false, true>(nwords, syms, mode, a, ysplit, stream);
}

}  // namespace edlib_amd
