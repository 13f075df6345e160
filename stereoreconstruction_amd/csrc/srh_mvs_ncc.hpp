// srh_mvs_ncc.hpp -- the arithmetic that parity of MultiViewStereo's matching cost and peak rule with the reference depends
// on, stated once and usable from host and gfx950 device code: the kernels (srh_mvs.hip, srh_mvs_subpixel.hip) say where
// the taps come from and where weights and a_t live, and the CPU suite compiles this header with g++ and holds it to the
// oracle bit for bit (tests/mvs_ncc_host.cpp, tests/test_mvs_ncc_host.py).
//
//   mvs_select_cost     the free cost_ncc (stereo/multiviewstereo.cpp:113-189) in its select form: any validity pattern,
//                       a skipped tap adds +0.0 to every sum -- sums of non-negative products never hold -0.0 and sum1
//                       starts at +0.0, so each partial sum keeps its bits and the selects are the reference's guards
//                       (mvs_select_cost_n: the same body for a window size known at run time only)
//   mvs_unit_constants  totalWeight, sum2 and a_t = w_t*gl_t - meanL of a reference window whose taps are all usable
//   mvs_fast_cost       the two sweeps of that form (mvs_fast_products, mvs_fast_sums: any run of taps) and the finish
//   mvs_peaks_init / mvs_peaks_insert / mvs_peak_better   :553 / :562, :600-602 and :589-594
//
// Everything is evaluated in the reference's order, one operation at a time: build without contraction.
#pragma once

#include "srh_ncc.hpp"                 // SRH_NHD, <math.h>

namespace srh {

// The one body.  The window arrives as `rows` x `cols` taps, row-major, CH taps at a time: taps(row, col0, gl, gr, wt) fills
// the CH taps of window row `row` from column col0 on (gl / gr = the reference / the other view's gray value, NaN = no
// such pixel; wt = the weights), once in either sweep.  CH = 1: no array that a run-time index would push out of registers.
template <int CH, class Taps>
SRH_NHD double mvs_select_cost_body(int rows, int cols, Taps &&taps, double weight_cutoff)
{
	double meanL = 0, meanR = 0, totalWeight = 0.0;
	for (int row = 0; row < rows; ++row)
		for (int c0 = 0; c0 < cols; c0 += CH) {
			double gl[CH], gr[CH], wt[CH];
			taps(row, c0, gl, gr, wt);
#pragma unroll
			for (int col = 0; col < CH; ++col) {
				const bool ok = gl[col] == gl[col] && gr[col] == gr[col] && wt[col] > weight_cutoff;
				const double pl = wt[col]*gl[col], pr = wt[col]*gr[col];
				meanL += ok ? pl : 0.0;
				meanR += ok ? pr : 0.0;
				totalWeight += ok ? wt[col] : 0.0;
			}
		}
	if (totalWeight < 1e-10) return 0;
	meanL /= totalWeight;
	meanR /= totalWeight;
	double sum1 = 0, sum2 = 0, sum3 = 0;
	for (int row = 0; row < rows; ++row)
		for (int c0 = 0; c0 < cols; c0 += CH) {
			double gl[CH], gr[CH], wt[CH];
			taps(row, c0, gl, gr, wt);
#pragma unroll
			for (int col = 0; col < CH; ++col) {
				const bool ok = gl[col] == gl[col] && gr[col] == gr[col] && wt[col] > weight_cutoff;
				const double a = wt[col]*gl[col] - meanL, b = wt[col]*gr[col] - meanR;
				const double ab = a*b, aa = a*a, bb = b*b;
				sum1 += ok ? ab : 0.0;
				sum2 += ok ? aa : 0.0;
				sum3 += ok ? bb : 0.0;
			}
		}
	if (sum2 * sum3 < 1e-10) return 0;
	return sum1 / sqrt(sum2 * sum3);
}

// A window of WS x WS taps that fits the registers: rows(row, gl, gr, wt) fills window row `row`, as for ncc_select_cost
// (srh_ncc.hpp).  The whole window is one chunk: the sweeps are unrolled over its taps.
template <int WS, class Rows>
SRH_NHD double mvs_select_cost(Rows &&rows, double weight_cutoff)
{
	return mvs_select_cost_body<WS*WS>(1, WS*WS, [&](int, int, double *gl, double *gr, double *wt) {
#pragma unroll
		for (int row = 0; row < WS; ++row) rows(row, gl + row*WS, gr + row*WS, wt + row*WS);
	}, weight_cutoff);
}

// any window size at run time: tap(row, col, gl, gr, wt) sets the three values of one tap
template <class Tap>
SRH_NHD double mvs_select_cost_n(int WS, Tap &&tap, double weight_cutoff)
{
	return mvs_select_cost_body<1>(WS, WS, [&](int row, int col, double *gl, double *gr, double *wt) { tap(row, col, gl[0], gr[0], wt[0]); }, weight_cutoff);
}

// The same cost once more, for mvs_unit_general (srh_mvs.hip): the whole window in registers and its usable taps known as
// a mask (ok[t] on entry: usable on the reference side and inside the other image; the other view's NaN is tested here).
// Routed through the body above, that function -- the redo of every silhouette pixel of a photograph -- ran 11 % slower
// (profiles/mvs_ncc_refactor_ab.txt); tests/mvs_ncc_host.cpp holds this form to mvs_select_cost bit for bit.
template <int T>
SRH_NHD double mvs_select_cost_masked(const double (&wt)[T], const double (&gl)[T], const double (&gr)[T], bool (&ok)[T])
{
	double mL = 0, mR = 0, twg = 0.0;
#pragma unroll
	for (int t = 0; t < T; ++t) {
		const bool o = ok[t] && gr[t] == gr[t];
		ok[t] = o;
		const double pl = wt[t]*gl[t], pr = wt[t]*gr[t];
		mL += o ? pl : 0.0; mR += o ? pr : 0.0; twg += o ? wt[t] : 0.0;
	}
	if (twg < 1e-10) return 0;
	mL /= twg;
	mR /= twg;
	double s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
	for (int t = 0; t < T; ++t) {
		const double aa = wt[t]*gl[t] - mL, bb = wt[t]*gr[t] - mR;
		const double ab = aa*bb, a2 = aa*aa, b2 = bb*bb;
		s1 += ok[t] ? ab : 0.0; s2 += ok[t] ? a2 : 0.0; s3 += ok[t] ? b2 : 0.0;
	}
	if (s2 * s3 < 1e-10) return 0;
	return s1 / sqrt(s2 * s3);
}

// ---- the all-taps-usable form: all = every tap of the reference window usable (gray value valid, weight above the
// cut-off), the caller's own precondition `all_seed` holds and totalWeight is not below 1e-10; then a_t = w_t*gl_t - meanL
// and s2 = sum2, neither of which depends on the candidate.
struct MvsUnit { double tw, s2; bool all; };

// tap(t, wt, gl) fetches tap t (row-major) of the reference window; w(t) is where the caller keeps weight t (registers,
// a column of LDS), a[] receives a_t.  Not all: a[] is left holding the gray values, or zeros with ZERO_A.
template <int T, bool ZERO_A, class Tap, class W>
SRH_NHD MvsUnit mvs_unit_constants(Tap &&tap, W &&w, double (&a)[T], double weight_cutoff, bool all_seed)
{
	bool all = all_seed;
	double mL = 0, tw = 0, s2 = 0;
#pragma unroll
	for (int t = 0; t < T; ++t) {
		double wt, gl;
		tap(t, wt, gl);
		all = all && gl == gl && wt > weight_cutoff;
		w(t) = wt;
		a[t] = gl;
		mL += wt*gl;
		tw += wt;
	}
	if (all && !(tw < 1e-10)) {
		mL /= tw;
#pragma unroll
		for (int t = 0; t < T; ++t) { a[t] = w(t)*a[t] - mL; s2 += a[t]*a[t]; }
	} else {
		all = false;
		if (ZERO_A) {
#pragma unroll
			for (int t = 0; t < T; ++t) a[t] = 0.0;
		}
	}
	return MvsUnit{ tw, s2, all };
}

// first sweep over taps [t0, t0 + N): g_t becomes p_t = w_t*g_t (multiviewstereo.cpp:150-151, 171), their sum goes onto mR
template <int N, class W>
SRH_NHD void mvs_fast_products(W &&w, double *g, int t0, double &mR)
{
#pragma unroll
	for (int t = t0; t < t0 + N; ++t) { g[t] = w(t)*g[t]; mR += g[t]; }
}

// second sweep over taps [t0, t0 + N), mR = meanR (the first sweep's sum / totalWeight)
template <int N>
SRH_NHD void mvs_fast_sums(const double *a, const double *p, int t0, double mR, double &s1, double &s3)
{
#pragma unroll
	for (int t = t0; t < t0 + N; ++t) {
		const double b = p[t] - mR;
		s1 += a[t]*b;
		s3 += b*b;
	}
}

// den = sum2 * sum3
SRH_NHD double mvs_fast_finish(double s1, double den) { return (den < 1e-10) ? 0.0 : s1 / sqrt(den); }

// the whole candidate: g[] holds the other view's window on entry and the products on return
template <int T, class W>
SRH_NHD double mvs_fast_cost(W &&w, const double (&a)[T], double (&g)[T], double tw, double s2)
{
	double mR = 0, s1 = 0, s3 = 0;
	mvs_fast_products<T>(w, g, 0, mR);
	mR /= tw;
	mvs_fast_sums<T>(a, g, 0, mR, s1, s3);
	return mvs_fast_finish(s1, s2 * s3);
}

// ---- A peak list: the K largest (cost, depth) pairs seen so far, ascending (multiviewstereo.cpp:600-602: sort, keep the last
// K); pk[0], pk[1] is the smallest kept pair.  It starts as K x (0, -1) (:553, :562).
SRH_NHD void mvs_peaks_init(double *pk, int K)
{
	for (int k = 0; k < K; ++k) { pk[2*k] = 0.0; pk[2*k + 1] = -1.0; }
}

// is (c, z) the larger pair?  std::sort's order on pairs: the cost first, an exact tie is decided by the depth (:589-594)
SRH_NHD bool mvs_peak_better(double c, double z, double bestC, double bestZ) { return c > bestC || (c == bestC && z > bestZ); }

SRH_NHD void mvs_peaks_insert(double *__restrict__ pk, int K, double c, double z)
{
	if (!mvs_peak_better(c, z, pk[0], pk[1])) return;
	int k = 0;
	while (k + 1 < K && mvs_peak_better(c, z, pk[2*(k + 1)], pk[2*(k + 1) + 1])) {
		pk[2*k] = pk[2*(k + 1)]; pk[2*k + 1] = pk[2*(k + 1) + 1];
		++k;
	}
	pk[2*k] = c; pk[2*k + 1] = z;
}

}  // namespace srh
