// srh_wta.hpp -- the decisions a TwoView depth map rests on, stated once and usable from host and gfx950 device code: the
// winner-take-all rule of TwoViewStereo::computeCostVolumes, its ratio test, and the doubt tests with which the certified
// scans decide whether those two comparisons, made on fused costs, are the reference's.  Every scan kernel calls it on its
// own loads and queues; the CPU suite compiles this header with g++ and holds the rule to the oracle bit for bit and the
// doubt tests to the property they are there for (tests/wta_host.cpp, tests/test_wta_host.py).
//
//   WtaState::take      `cost + wta_margin < minCost` -> secondBest = minCost, minCost = cost, winner = candidate
//                       (stereo/twoviewstereo.cpp:293-301)
//   WtaState::rejected  `minCost > second_best_factor*secondBest` -> depth = +inf (:304-305)
//   cert_step_doubt     is a step's comparison on stored costs possibly not the reference's?
//   cert_ratio_doubt    the same for the ratio test
//   CertBound, cert_bound, cert_sure, cert_pixel_exact   the certificate's numbers (bound: DESIGN.md section 2b)
//
// Everything is evaluated in the reference's order, one operation at a time: build without contraction.
#pragma once

#include <math.h>
#include <stdint.h>

#include "stereo_recon_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef SRH_NHD                        // (srh_ncc.hpp has the same definition)
#if defined(__HIPCC__)
#define SRH_NHD __host__ __device__ __forceinline__
#else
#define SRH_NHD inline
#endif
#endif

namespace srh {

// ---- the rule -------------------------------------------------------------------------------------------------------
// A candidate pixel of the other view as the general kernel carries it; the row-aligned kernels carry a column (int), the
// list kernels the packed y << 16 | x (uint32_t).
struct WtaXY {
	int x, y;
	SRH_NHD bool operator==(const WtaXY &o) const { return x == o.x && y == o.y; }
	SRH_NHD bool operator!=(const WtaXY &o) const { return !(*this == o); }
};

// The state of one reference pixel's scan (:280-281).  Id names a candidate; `none` is the site's "no candidate yet".
// run: the candidate that held minCost immediately before the last improvement (its cost is secondBest); kept only with
// WTA (option "wta_outputs"), else it stays `none`.
template <class Id, bool WTA>
struct WtaState {
	double minCost, secondBest;
	Id win, run;
	SRH_NHD explicit WtaState(Id none) : minCost(__builtin_inf()), secondBest(__builtin_inf()), win(none), run(none) {}
	// t: the caller's cost + margin (a site that needs t for the doubt test as well, or that turns a lane off with t = +inf)
	SRH_NHD void take_sum(double t, double cost, Id id) {
		if (t < minCost) {                                     // :293
			secondBest = minCost;                              // :298
			minCost = cost;                                    // :299
			if (WTA) run = win;
			win = id;                                          // (:294-300: the depth written is the winner's, geometry)
		}
	}
	SRH_NHD void take(double cost, Id id, double margin) { take_sum(cost + margin, cost, id); }
	// :304-305.  Without a winner both are +inf and the verdict is false.
	SRH_NHD bool rejected(double factor) const { return minCost > factor*secondBest; }
};

// ---- certified fused arithmetic (option "arith" = 3; derivation of the bound: DESIGN.md section 2b) -------------------------
// The dense cost loops run with fused multiply-adds (half the FP64 instructions); a depth map depends on costs only
// through comparisons (the two above and the max_color_diff clamp, twoviewstereo.cpp:976), so the fused costs may stand in
// for the reference's wherever no comparison's margin is inside the error bound.  For a fast-form candidate (all T taps
// usable; weights in (0,1] -- or up to wmax, see cert_bound --, grays in [0,255]; meanL, totalWeight and sum2 are the SAME bits in both arithmetics), with
// u = 2^-53, gamma_k = k*u/(1-k*u), G = 256, A = sqrt(sum2), B = sqrt(sum3):
//     eps_b = gamma_(T+4)*G   (error of w*g_R - meanR: the mean's T-term sum and division, the product, the subtraction)
//     eps_a = 2*u*G           (error of w*g_L - meanL: meanL is shared)
//     |cost_fused - cost_exact| <= 2*255*1.01*(3*eps_b*sqrt(T)/B + eps_a*sqrt(T)/A + 2*gamma_T) + 2600*u
//                                =  k1/B + k2/A + k3
// (either arithmetic is within half of that of the real-number value of the formula; 1.01 covers every second-order
// term wherever the bound is used).  A candidate is CERTIFIED when that is <= e0, i.e. when sum3 >= sigma3(sum2); the cost
// kernel stores NaN for the others.
// ONE-PASS form (strip kernel, AR = 5).  Nothing obliges the fused kernel to follow the reference's two sweeps: any
// arithmetic within e0 of the reference's will do.  With c_t = (w_t*l_t - meanL)*w_t, d_t = w_t^2, q = r^2 it accumulates
// P = sum w_t r_t, Q = sum c_t r_t, U = sum d_t q_t in ONE sweep over the window (3 fused multiply-adds per tap and
// candidate instead of 4, and 40 instead of 69 LDS values per window row and block), and finishes with m = P/tw,
// sum3 = U - m*(2P - T*m), sum1 = Q - m*SA (SA = sum of w_t*l_t - meanL).  The price is cancellation in sum3: with
// Q3 = U + 2mP + T*m^2 (every term >= 0) and z^2 = Q3/sum3, the one-pass value is within
//     255*1.01*(3*gamma_(T+4)*z + 2.002*gamma_(T+3)*z^2) + 1300u
// of the real-number cost, the reference's arithmetic within half of k1/B + k2/A + k3: a candidate is
// certified when sum3 >= sigma3(sum2) (the latter <= e0/2) and Q3 <= zmax2*sum3 (the former <= e0/2).
// The FINISH of a one-pass candidate is free of IEEE divisions and of the IEEE square root as well (onepass_finish,
// srh_block.hpp): m = P*itw with itw = fl(1/tw) from the weights kernels (one more rounding on m: every gamma index of
// the derivation goes up by one; the code takes gamma_(T+6) for both terms), 1/sqrt(sum2*sum3) by v_rsq_f64 and ONE
// third-order Newton step whose own residual e = 1 - x*y0^2 is part of the certificate (|e| <= 2^-20, whatever the seed's
// accuracy: y1 = y0*(1 + e/2 + 3e^2/8) is then within 2u of 1/sqrt(x)), and v = fma(-255, |sum1|*y1, 255): x, the product
// and the last fma round once each, so the finish's share of the bound is 255*1.001*(0.5u + 2u + u) + 255u < 1150u; the
// constant stays at 2600u.
struct CertBound {
	double e0, m_hi, k1, k2, room;
	double zmax2;
	int ok;                                 // 0: the parameters leave the bound no room / weights are not in (0, wmax]: exact arithmetic
	SRH_NHD double sigma3(double s2) const {
		const double d = room - k2/sqrt(s2);                      // (NaN or zero sum2: d is NaN or -inf)
		if (!(d > 0)) return __builtin_inf();
		const double b = k1/d;
		return b*b*(1.0 + 0x1p-20);                               // (+ the roundings of this very computation)
	}
};
// mvs: the free cost_ncc of MultiViewStereo (multiviewstereo.cpp:113-189): the score sum1/sqrt(sum2*sum3) itself (no factor
// 255, no clamp), 25 taps at the reference's radius; e0 = 2^-36 there (scores live in [-1, 1])
inline CertBound cert_bound(const srh_params &P, bool mvs = false) {
	// Weights above 1: a geodesic window started below zero (geodesic_init < 0, sigma > 0) keeps geodesic_init on every tap but
	// the centre, whose distance stays in [geodesic_init, 0]: weights in [1, wmax], wmax = exp(-geodesic_init/geodesic_sigma).
	// The derivation sees the weights only through G, the bound of |weight*gray|: eps_a and eps_b, hence k1 and k2, are
	// linear in it; k3 and the one-pass form's z^2 = Q3/sum3 are ratios that a common factor of the weights leaves alone.
	// So G = 256*wmax covers them (sum2 and sum3 grow by wmax^2 with it: as many candidates certify as at wmax = 1), up to
	// the magnitude the other parameters are held to (wmax <= 1e5: no sum comes near the range's end).  With G = 256 the
	// test sum3 >= sigma3(sum2) would admit bounds up to wmax*e0.
	const bool geo = P.weight_kind == SRH_WEIGHT_GEODESIC;
	const double wmax = geo && P.geodesic_sigma > 0 && P.geodesic_init < 0 ? exp(-P.geodesic_init/P.geodesic_sigma) : 1.0;
	const double u = 0x1p-53, G = 256.0*wmax;
	const int T = (2*P.window_radius + 1)*(2*P.window_radius + 1);
	auto gamma = [&](int k) { return k*u/(1.0 - k*u); };
	const double eps_b = gamma(T + 4)*G, eps_a = 2*u*G, rt = sqrt((double)T);
	const double scale = mvs ? 1.0 : 255.0;
	CertBound c;
	c.e0 = mvs ? 0x1p-36 : 0x1p-26;                               // TwoView: 1.5e-8, a comparison needs 3.7e-8 of margin (costs live in [0, 120])
	c.k1 = 2*scale*1.01*3*eps_b*rt;
	c.k2 = 2*scale*1.01*eps_a*rt;
	const double k3 = 2*scale*1.01*2*gamma(T) + (mvs ? 40 : 2600)*u;
	c.room = c.e0 - k3;
	c.m_hi = P.max_color_diff + c.e0;
	{	// one-pass form: 255*1.01*g*(3z + 2.002 z^2) + 2600u = e0/2  (g = gamma_(T+6): the finish multiplies by fl(1/tw))
		const double g = gamma(T + 6), rhs = (c.e0/2 - 2600*u)/(scale*1.01*g);
		const double z = rhs > 0 ? (-3.0 + sqrt(9.0 + 4*2.002*rhs))/(2*2.002) : 0.0;
		c.zmax2 = z*z*(1.0 - 0x1p-20);
	}
	const bool weights_ok = geo ? P.geodesic_sigma > 0 && wmax <= 1e5 : P.adaptive_color_sigma > 0;   // exp(-distance/sigma) <= 1 (geodesic: <= wmax)
	if (mvs) { c.ok = c.room > 0 && weights_ok && fabs(P.peak_threshold) <= 1e5; return c; }
	// what the doubt tests below assume of the parameters: max_color_diff + e0 > max_color_diff (so below 2^22),
	// wta_margin >= 0, and magnitudes <= 1e5
	c.ok = c.room > 0 && c.m_hi > P.max_color_diff && P.max_color_diff <= 1e5 && fabs(P.bad_ret) <= 1e5 &&
	       P.wta_margin >= 0 && P.wta_margin <= 1e5 && fabs(P.second_best_factor) <= 1e5 && weights_ok;
	return c;
}

// ---- the doubt tests --------------------------------------------------------------------------------------------------
// What a stored value x of a certified cost kernel says about the cost c in the reference's arithmetic:
//   x > max_color_diff + e0                           c == x, the very same number ("sure", cert_sure): such values
//                                                     (bad_ret) come from the select forms, which every mode evaluates
//                                                     in the reference's arithmetic;
//   x == max_color_diff                               read as sure as well.  That is proved when the kernel PUT the clamp
//                                                     there -- it does so only for a fused value above clamp + e0, and
//                                                     the clamp is 1-Lipschitz, so c is the clamp -- or when a select
//                                                     form computed it.  It is NOT proved for a fused value whose own
//                                                     bits are the clamp's: the kernels store it as it is (block_stored,
//                                                     srh_block.hpp: the one statement of the rule), and c may lie
//                                                     up to e0 below it.  A GAP of the certificate, the parent's
//                                                     behaviour, left as it is; tests/test_wta_host.py keeps the case
//                                                     (test_fused_cost_equal_to_the_clamp, a strict xfail);
//   x NaN                                             an uncertified candidate: nothing is known, the pixel is flagged;
//   anything else                                     |x - c| <= e0 (select-form candidates are exact and counted as e0;
//                                                     a fused value in (clamp, clamp + e0] stands for a c in [x - e0, clamp]).
// The scan replays the reference's loop on the stored values.  Outside that gap: if every comparison it makes comes out as the reference's
// own comparison on the c's, then by induction over the candidate sequence the state -- winner, runner-up, and WHICH
// candidates' costs sit in minCost and secondBest -- evolves identically: minCost and secondBest are themselves stored
// values of earlier candidates (or the initial +inf, which is sure), so the table above applies to them as well.  The
// depth written is a function of the winner (geometry) and of the ratio verdict, hence the reference's bits.  A pixel
// with a comparison that is not certainly the reference's is FLAGGED and redone in the reference's arithmetic.
//
// A step compares t = fl(x + margin) with minCost; the reference compares fl(c + margin) with its minCost.  The two left
// sides differ by at most e0 + the two roundings, the right sides by at most e0.  An unsure side is a cost, a clamp or a
// bad_ret of magnitude <= 1e5 and so is the margin (CertBound::ok), so each rounding is at most u*2e5 < e0/4: the four
// quantities move the difference t - minCost by less than 2*e0 + e0/2, and a difference beyond 2.5*e0 has the reference's
// sign.  Within 2.5*e0 the comparison is still the reference's
//   - when both sides are sure: the same numbers go through the same operations;
//   - when the candidate IS the current winner, seen again (curves revisit pixels at segment joints): both arithmetics
//     compare a cost + margin with that very cost, false in either while wta_margin >= 0 (CertBound::ok; a negative margin
//     would let a revisited winner "beat" itself and move secondBest);
//   - when px_sure: the cost kernel evaluated this whole pixel in the reference's arithmetic (cert_pixel_exact: unusable
//     taps of its own, or a window that leaves the bound no room), so every stored number that is a number is c itself.
//     A NaN is flagged whatever the pixel.  What px_sure buys: without it every near-tie of such a pixel -- and flat or
//     saturated regions consist of them -- would go to the redo for costs that are exact already.
// Only the strip kernel redoes pixels in place, so only its scans (the per-tile and the template scan, given the band's
// pixel constants) know a px_sure pixel.  The row-run scan passes px_sure = false: its cost kernel stores NaN for every
// candidate the bound does not cover and evaluates no pixel exactly throughout, so no pixel's stored costs are known to
// be the reference's as a whole.
SRH_NHD bool cert_sure(double x, double clamp, double m_hi) { return x == clamp || x > m_hi; }
// a pixel with unusable taps of its own (every candidate in a select form) or whose own window leaves the bound no room
// (sigma3 = +inf): the strip kernel evaluates it in the reference's arithmetic throughout
SRH_NHD bool cert_pixel_exact(const CertBound &cb, double sum2, double all_taps_usable) {
	return !(all_taps_usable != 0.0) || !(cb.sigma3(sum2) < __builtin_inf());
}
// the first clause of the step's test on its own (NaN: near): almost always false, so a wave may skip the rest together
SRH_NHD bool cert_step_near(double t, double minCost, const CertBound &cb) { return !(fabs(t - minCost) > 2.5*cb.e0); }
// cost: the stored value x; t = x + margin; is_winner: the candidate is the state's current winner
SRH_NHD bool cert_step_doubt(double cost, double t, double minCost, bool is_winner, bool px_sure, const CertBound &cb, double clamp) {
	return cert_step_near(t, minCost, cb) && !is_winner &&
	       !(cert_sure(cost, clamp, cb.m_hi) && cert_sure(minCost, clamp, cb.m_hi)) &&
	       !(px_sure && cost == cost);
}
// The ratio test compares minCost (within e0) with fl(factor*secondBest): within |factor|*e0 of the reference's product
// before rounding, and each rounding is at most u*|rhs| -- the 1e-15*|rhs| term (capped so that an infinite secondBest
// leaves a finite tolerance and an infinite difference).  For a pixel with a winner; sure on both sides, or px_sure, as
// above (a NaN never enters the state, and has flagged the pixel already).
SRH_NHD bool cert_ratio_doubt(double minCost, double secondBest, double factor, bool px_sure, const CertBound &cb, double clamp) {
	const double rhs = factor*secondBest;
	const double tol = __builtin_fma(fmin(fabs(rhs), 1e300), 1e-15, (1.0 + fabs(factor))*cb.e0);
	return !(fabs(minCost - rhs) > tol) && !px_sure &&
	       !(cert_sure(minCost, clamp, cb.m_hi) && cert_sure(secondBest, clamp, cb.m_hi));
}

}  // namespace srh
