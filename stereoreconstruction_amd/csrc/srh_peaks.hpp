// srh_peaks.hpp -- the label space of MultiViewStereo's MRF branch, K collected peaks + "unknown" with one label per lane
// and 16 lanes per pixel: what srh_mrf.hip (TRW-S) and srh_mvs_sgm.hip (semi-global aggregation) share.
//   bc16<I>          a pixel's value of label I in all 16 lanes of the pixel (DPP row broadcast: no LDS)
//   smooth_peak      smoothnessCost (multiviewstereo.cpp:499-514) between a peak label of one pixel and a label of another
//   smooth_carried   the same with the first label given as a carried value
#pragma once
#include <hip/hip_runtime.h>

namespace srh {

namespace {

template <int I> __device__ __forceinline__ double bc16(double v) {
	return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + I, 0xf, 0xf, false);      // row_newbcast:I
}

// smoothnessCost (multiviewstereo.cpp:499-514) between a peak label of one pixel (depth z1) and label kd of another (z2)
// (written as selects over an unconditional quotient: the divisions of one step are independent of each other and of
// the messages, and only straight-line code lets the scheduler overlap them)
__device__ __forceinline__ double smooth_peak(double z1, double z2, bool kd_unknown, double psi, double psi2) {
	const double q = 2.0 * fabs(z1 - z2) / (z1 + z2);
	const double r = (z1 < 0 || z2 < 0) ? psi2 : q;
	return kd_unknown ? psi : r;
}
// the same with the first label given as a carried value: NaN = "unknown", otherwise that label's depth
__device__ __forceinline__ double smooth_carried(double c, double z2, bool kd_unknown, double psi, double psi2) {
	if (c != c) return kd_unknown ? 0.0 : psi;
	return smooth_peak(c, z2, kd_unknown, psi, psi2);
}

} // namespace

} // namespace srh
