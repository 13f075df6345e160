// srh_ncc.hpp -- the arithmetic that parity of the TwoView NCC cost with the reference depends on, stated once and
// usable from host and gfx950 device code: the kernels call it with a callable that says where a window row's taps
// come from (pointers and strides, LDS tiles, a ring of rows, float tiles, bounds-checked gathers), and the CPU suite
// compiles this header with g++ and holds it to the oracle bit for bit (tests/ncc_host.cpp, tests/test_ncc_host.py).
//
//   ncc_select_cost   TwoViewStereo::cost_ncc (stereo/twoviewstereo.cpp:909-977) in its select form: any validity
//                     pattern, a skipped tap adds +0.0 to every sum -- which leaves each partial sum bit for bit
//                     unchanged, so the selects are the reference's "continue" (:920-938, :955-972)
//   pixel_constants   meanL, totalWeight, sum2 (and SA of the one-pass form) of :917-976 for a window whose every tap
//                     is usable: they do not depend on the candidate (the fast form)
//   pconst_store      the per-pixel record of those constants in the `pconst` buffer
//
// Everything is evaluated in the reference's order, one operation at a time: build without contraction.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef SRH_NHD                        // (srh_wta.hpp has the same definition)
#if defined(__HIPCC__)
#define SRH_NHD __host__ __device__ __forceinline__
#else
#define SRH_NHD inline
#endif
#endif

namespace srh {

// rows(row, gl, gr, wt) fills window row `row`: gl / gr = the reference / the other view's tap values (NaN = unusable),
// wt = the weights.  Loops by window row so that a row's loads travel together.
template <int WS, class Rows>
SRH_NHD double ncc_select_cost(Rows &&rows, double weight_cutoff, double bad_ret, double max_color_diff)
{
	double meanL = 0, meanR = 0, totalWeight = 0.0;
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		double gl[WS], gr[WS], wt[WS];
		rows(row, gl, gr, wt);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const bool ok = gl[col] == gl[col] && gr[col] == gr[col] && wt[col] > weight_cutoff;
			const double pl = wt[col]*gl[col], pr = wt[col]*gr[col];
			meanL += ok ? pl : 0.0;
			meanR += ok ? pr : 0.0;
			totalWeight += ok ? wt[col] : 0.0;
		}
	}
	if (totalWeight < 1e-10) return bad_ret;
	meanL /= totalWeight;
	meanR /= totalWeight;
	double sum1 = 0, sum2 = 0, sum3 = 0;
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		double gl[WS], gr[WS], wt[WS];
		rows(row, gl, gr, wt);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const bool ok = gl[col] == gl[col] && gr[col] == gr[col] && wt[col] > weight_cutoff;
			const double a = wt[col]*gl[col] - meanL, b = wt[col]*gr[col] - meanR;
			const double ab = a*b, aa = a*a, bb = b*b;
			sum1 += ok ? ab : 0.0;
			sum2 += ok ? aa : 0.0;
			sum3 += ok ? bb : 0.0;
		}
	}
	const double v = 255*(1.0 - fabs(sum1) / sqrt(sum2 * sum3));
	return (v < max_color_diff) ? v : max_color_diff;
}

// all: every tap usable (gray value valid, weight above the cut-off) and totalWeight not below 1e-10; then mL is meanL,
// s2 is sum2 and sa the sum of fma(w, l, -meanL) (the one-pass form's SA, fused terms).  Otherwise mL is the undivided
// sum of w*l and s2 = sa = 0.
struct PixelConstants { double mL, tw, s2, sa; bool all; };

// The second sweep, from the first one's sums: mL = sum of w*l, tw = sum of w over window rows [ra, rb), taps row-major;
// all = the caller's own precondition and every tap usable.  rows(row, gl, wt) as above, without the other view.
template <int WS, bool SA, class Rows>
SRH_NHD PixelConstants pixel_constants_finish(Rows &&rows, double mL, double tw, bool all, int ra = 0, int rb = WS)
{
	double s2 = 0, sa = 0;
	if (all && !(tw < 1e-10)) {
		mL /= tw;
#pragma unroll 1
		for (int row = ra; row < rb; ++row) {
			double gl[WS], wt[WS];
			rows(row, gl, wt);
#pragma unroll
			for (int col = 0; col < WS; ++col) {
				const double t = wt[col]*gl[col] - mL;
				s2 += t*t;
				if (SA) sa += __builtin_fma(wt[col], gl[col], -mL);
			}
		}
	} else all = false;
	return PixelConstants{ mL, tw, s2, sa, all };
}

// Both sweeps over window rows [ra, rb).  all_seed: the caller's own precondition (the pixel lies in the image, has
// candidates ...); it enters before the test of totalWeight, so a false seed leaves the undivided mL and s2 = 0.
template <int WS, bool SA, class Rows>
SRH_NHD PixelConstants pixel_constants(Rows &&rows, double weight_cutoff, bool all_seed, int ra = 0, int rb = WS)
{
	bool all = all_seed;
	double mL = 0, tw = 0;
#pragma unroll 1
	for (int row = ra; row < rb; ++row) {
		double gl[WS], wt[WS];
		rows(row, gl, wt);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			if (!(gl[col] == gl[col] && wt[col] > weight_cutoff)) all = false;
			mL += wt[col]*gl[col];
			tw += wt[col];
		}
	}
	return pixel_constants_finish<WS, SA>(rows, mL, tw, all, ra, rb);
}

// the six slots of a pixel's record (SRH_PC of srh_internal.hpp)
SRH_NHD void pconst_store(double *pc, const PixelConstants &c)
{
	pc[0] = c.mL; pc[1] = c.tw; pc[2] = c.s2;
	pc[3] = c.all ? 1.0/c.tw : 0.0;   // all taps usable: != 0, and then 1/totalWeight (the one-pass form multiplies by it)
	pc[4] = c.sa; pc[5] = 0.0;
}

}  // namespace srh
