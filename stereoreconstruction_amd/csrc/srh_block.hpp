// srh_block.hpp -- the FAST-FORM BLOCK of the TwoView NCC cost, stated once and usable from host and gfx950 device code:
// NCB adjacent candidates of one reference pixel whose taps are all usable on both sides, evaluated over the window by
// row loops that are modulo-scheduled by hand.  The cost kernels (twoview_strip_cost_kernel, twoview_dense_cost_kernel,
// twoview_rows_cost_kernel, twoview_fused_kernel) call it with a ROW SOURCE that says where a window row comes from; the
// CPU suite compiles this header with g++ and holds it to ncc_select_cost of srh_ncc.hpp -- itself held to the oracle --
// and to the certificate of srh_wta.hpp (tests/block_host.cpp, tests/test_block_host.py).
//
//   block_two_sweeps   the reference's two sweeps (stereo/twoviewstereo.cpp:917-976: products first, sums second) over
//                      window rows [ra, rb), or the same with fused multiply-adds (FMA): sum1 and sum3 of each candidate
//   block_onepass      the certified one-pass form's sums P = sum w r, Q = sum ((w l - meanL) w) r, U = sum w^2 r^2
//   block_onepass_taps the same sums, the tap products (w l - meanL) w read from the source instead of built per block
//   two_sweep_finish   255*(1 - |sum1|/sqrt(sum2*sum3))
//   onepass_finish     the one-pass cost from P, Q, U without an IEEE division or square root, and its certificate
//   block_stored       what a cost kernel stores for a fast-form candidate: the clamped value (exact forms) or NaN, the
//                      clamp or the value (certified forms)
//
// A row source is a struct of forceinline members, one type per site, defined next to its kernel:
//   static constexpr bool LDS_WAIT   an `s_waitcnt lgkmcnt(0)` stands before each row loop (the pre-header's LDS reads have
//                                    landed: inside the loop the compiler then counts only the previous iteration's reads)
//   Row row(int row) const           the cursor of window row `row`:
//       void r2(int m, double &a, double &b)   values 2m, 2m + 1 of the other view's segment of NCB + WS - 1 values (a pair
//                                              read at an even index, two 8-byte reads, or a global pointer)
//       void w2(int m, double &a, double &b)   weights 2m, 2m + 1 of the row;   double w(int col)   one weight
//       double l(int col)                      the reference view's tap
//       void c2(int m, double &a, double &b), double c(int col)   (sources of block_onepass_taps only, which need no l)
//                                              the tap products fma(w, l, -meanL)*w, addressed like the weights
//   int row_begin(int units), void row_end(int seen)   what runs at the start and the end of a window row (the strip
//                                    kernel publishes its progress and yields to its SIMD partner; nothing elsewhere)
// The schedule: the pre-header fills r[] and wv[] with the first row; a value's register is refilled with the NEXT row's
// value right after its last use, so the loads are always a row ahead; products before sums, so that no instruction waits
// on its predecessor; SRH_SCHED_BARRIER keeps each refill where it is written.  The last refill of the first sweep is row
// `ra` again, for the second sweep.
//
// Not here: the packed-single loops of srh_dense_f32.hip, the SAD blocks of srh_sad_strip.hip, the MultiViewStereo staged
// kernel, and the select forms (any validity pattern), which are in srh_ncc.hpp.
//
// Everything is evaluated one operation at a time, fused only where __builtin_fma is written: build without contraction.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef SRH_NHD                        // (srh_ncc.hpp and srh_wta.hpp have the same definition)
#if defined(__HIPCC__)
#define SRH_NHD __host__ __device__ __forceinline__
#else
#define SRH_NHD inline
#endif
#endif
// the scheduling fence and the LDS wait of the row loops: nothing on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define SRH_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#define SRH_LDS_WAIT() __builtin_amdgcn_s_waitcnt(0xC07F)        /* lgkmcnt(0) */
#else
#define SRH_SCHED_BARRIER() do { } while (0)
#define SRH_LDS_WAIT() do { } while (0)
#endif

namespace srh {

// sum1[j], sum3[j] of candidates j = 0 .. NCB - 1 over window rows [ra, rb); mL = meanL, tw = totalWeight of the pixel over
// the same rows (pixel_constants of srh_ncc.hpp).  Constant bounds fold: the callers outside the strip kernel's border
// instantiation pass 0 and WS.
// The source goes by value and the sums are accumulated in arrays of the function's own, copied out once at the end:
// accumulated through the references, or with the source behind one, the kernels' register allocation moves (the
// row-run kernel, at its 256 registers, then spills more) -- profiles/README.md has the numbers.
template <int WS, int NCB, bool FMA, class Src>
SRH_NHD void block_two_sweeps(const Src src, int ra, int rb, double mL, double tw, double (&sum1)[NCB], double (&sum3)[NCB])
{
	constexpr int NR = NCB + WS - 1;
	static_assert(WS % 2 == 1 && NR % 2 == 0, "odd window, the other view's segment in pairs");
	double r[NR], wv[WS], acc[NCB];
	{
		const auto first = src.row(ra);
#pragma unroll
		for (int m = 0; m < NR/2; ++m) first.r2(m, r[2*m], r[2*m + 1]);
#pragma unroll
		for (int m = 0; m < (WS - 1)/2; ++m) first.w2(m, wv[2*m], wv[2*m + 1]);
		wv[WS - 1] = first.w(WS - 1);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) acc[j] = 0.0;
	if (Src::LDS_WAIT) SRH_LDS_WAIT();
#pragma unroll 1
	for (int row = ra; row < rb; ++row) {
		const int seen = src.row_begin(1);
		const auto next = src.row(row + 1 < rb ? row + 1 : ra);       // last refill = row ra, for the second sweep
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			if (FMA) {
#pragma unroll
				for (int j = 0; j < NCB; ++j) acc[j] = __builtin_fma(wv[col], r[col + j], acc[j]);
			} else {
				double pr[NCB];
#pragma unroll
				for (int j = 0; j < NCB; ++j) pr[j] = wv[col]*r[col + j];
				SRH_SCHED_BARRIER();
#pragma unroll
				for (int j = 0; j < NCB; ++j) acc[j] += pr[j];            // meanR += weight*gray
			}
			SRH_SCHED_BARRIER();
			if (col & 1) {                                                // r[col-1], r[col], wv[col-1], wv[col] are dead
				next.r2(col >> 1, r[col - 1], r[col]);
				next.w2(col >> 1, wv[col - 1], wv[col]);
				SRH_SCHED_BARRIER();
			}
		}
#pragma unroll
		for (int m = (WS - 1)/2; m < NR/2; ++m) next.r2(m, r[2*m], r[2*m + 1]);
		wv[WS - 1] = next.w(WS - 1);
		src.row_end(seen);
	}
	double mR[NCB], s1[NCB], s3[NCB], av[WS];
	{
		const auto first = src.row(ra);
#pragma unroll
		for (int col = 0; col < WS; ++col) av[col] = first.l(col);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { mR[j] = acc[j]/tw; s1[j] = 0.0; s3[j] = 0.0; }
	if (Src::LDS_WAIT) SRH_LDS_WAIT();
#pragma unroll 1
	for (int row = ra; row < rb; ++row) {
		const int seen = src.row_begin(3);
		const auto next = src.row(row + 1 < rb ? row + 1 : ra);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const double wt = wv[col];
			if (FMA) {
				const double a = __builtin_fma(wt, av[col], -mL);
				double bb[NCB];
#pragma unroll
				for (int j = 0; j < NCB; ++j) bb[j] = __builtin_fma(wt, r[col + j], -mR[j]);
				SRH_SCHED_BARRIER();
#pragma unroll
				for (int j = 0; j < NCB; ++j) { s1[j] = __builtin_fma(a, bb[j], s1[j]); s3[j] = __builtin_fma(bb[j], bb[j], s3[j]); }
			} else {
				double bb[NCB], u1[NCB], u3[NCB];
				const double pa = wt*av[col];
#pragma unroll
				for (int j = 0; j < NCB; ++j) bb[j] = wt*r[col + j];
				SRH_SCHED_BARRIER();
				const double a = pa - mL;                                 // pixel_gray_l - meanL
#pragma unroll
				for (int j = 0; j < NCB; ++j) bb[j] = bb[j] - mR[j];      // pixel_gray_r - meanR
				SRH_SCHED_BARRIER();
#pragma unroll
				for (int j = 0; j < NCB; ++j) { u1[j] = a*bb[j]; u3[j] = bb[j]*bb[j]; }
				SRH_SCHED_BARRIER();
#pragma unroll
				for (int j = 0; j < NCB; ++j) { s1[j] += u1[j]; s3[j] += u3[j]; }
			}
			SRH_SCHED_BARRIER();
			av[col] = next.l(col);
			if (col & 1) {
				next.r2(col >> 1, r[col - 1], r[col]);
				next.w2(col >> 1, wv[col - 1], wv[col]);
			}
			SRH_SCHED_BARRIER();
		}
#pragma unroll
		for (int m = (WS - 1)/2; m < NR/2; ++m) next.r2(m, r[2*m], r[2*m + 1]);
		wv[WS - 1] = next.w(WS - 1);
		src.row_end(seen);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { sum1[j] = s1[j]; sum3[j] = s3[j]; }
}

// P[j], Q[j], U[j] of candidates j = 0 .. NCB - 1 over the whole window; q = r^2 is built a column ahead of its use.
// (Source by value, sums in the function's own arrays: as above.)
template <int WS, int NCB, class Src>
SRH_NHD void block_onepass(const Src src, double mL, double (&Pout)[NCB], double (&Qout)[NCB], double (&Uout)[NCB])
{
	double P[NCB], Q[NCB], U[NCB];
	constexpr int NR = NCB + WS - 1;
	static_assert(WS % 2 == 1 && NR % 2 == 0, "odd window, the other view's segment in pairs");
	double r[NR], q[NR], wv[WS], lv[WS];
	{
		const auto first = src.row(0);
#pragma unroll
		for (int m = 0; m < NR/2; ++m) first.r2(m, r[2*m], r[2*m + 1]);
#pragma unroll
		for (int m = 0; m < (WS - 1)/2; ++m) first.w2(m, wv[2*m], wv[2*m + 1]);
		wv[WS - 1] = first.w(WS - 1);
#pragma unroll
		for (int col = 0; col < WS; ++col) lv[col] = first.l(col);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { P[j] = 0.0; Q[j] = 0.0; U[j] = 0.0; }
	if (Src::LDS_WAIT) SRH_LDS_WAIT();
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const int seen = src.row_begin(4);
		const auto next = src.row(row + 1 < WS ? row + 1 : 0);            // (the last refill is never used)
#pragma unroll
		for (int k = 0; k < NCB - 1; ++k) q[k] = r[k]*r[k];
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			q[col + NCB - 1] = r[col + NCB - 1]*r[col + NCB - 1];
			const double a = __builtin_fma(wv[col], lv[col], -mL);
			const double c = a*wv[col], d = wv[col]*wv[col];
			SRH_SCHED_BARRIER();
#pragma unroll
			for (int j = 0; j < NCB; ++j) P[j] = __builtin_fma(wv[col], r[col + j], P[j]);
#pragma unroll
			for (int j = 0; j < NCB; ++j) Q[j] = __builtin_fma(c, r[col + j], Q[j]);
#pragma unroll
			for (int j = 0; j < NCB; ++j) U[j] = __builtin_fma(d, q[col + j], U[j]);
			SRH_SCHED_BARRIER();
			lv[col] = next.l(col);
			if (col & 1) {
				next.r2(col >> 1, r[col - 1], r[col]);
				next.w2(col >> 1, wv[col - 1], wv[col]);
			}
			SRH_SCHED_BARRIER();
		}
#pragma unroll
		for (int m = (WS - 1)/2; m < NR/2; ++m) next.r2(m, r[2*m], r[2*m + 1]);
		wv[WS - 1] = next.w(WS - 1);
		src.row_end(seen);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { Pout[j] = P[j]; Qout[j] = Q[j]; Uout[j] = U[j]; }
}

// The same sums from a source that SUPPLIES the tap products c_t = fma(w_t, l_t, -meanL)*w_t -- block_onepass's two
// operations, in its order, done once per pixel instead of in every block of it (the strip kernel's 8-wave form keeps them
// in LDS per tile): the same bits.  cv[] lives in the registers lv[] held and is refilled a row ahead with the weights; per
// tap only d = w^2 is left.  A function of its own: block_onepass's text, and its callers' code, stay what they are.
template <int WS, int NCB, class Src>
SRH_NHD void block_onepass_taps(const Src src, double (&Pout)[NCB], double (&Qout)[NCB], double (&Uout)[NCB])
{
	double P[NCB], Q[NCB], U[NCB];
	constexpr int NR = NCB + WS - 1;
	static_assert(WS % 2 == 1 && NR % 2 == 0, "odd window, the other view's segment in pairs");
	double r[NR], q[NR], wv[WS], cv[WS];
	{
		const auto first = src.row(0);
#pragma unroll
		for (int m = 0; m < NR/2; ++m) first.r2(m, r[2*m], r[2*m + 1]);
#pragma unroll
		for (int m = 0; m < (WS - 1)/2; ++m) { first.w2(m, wv[2*m], wv[2*m + 1]); first.c2(m, cv[2*m], cv[2*m + 1]); }
		wv[WS - 1] = first.w(WS - 1);
		cv[WS - 1] = first.c(WS - 1);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { P[j] = 0.0; Q[j] = 0.0; U[j] = 0.0; }
	if (Src::LDS_WAIT) SRH_LDS_WAIT();
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const int seen = src.row_begin(4);
		const auto next = src.row(row + 1 < WS ? row + 1 : 0);            // (the last refill is never used)
#pragma unroll
		for (int k = 0; k < NCB - 1; ++k) q[k] = r[k]*r[k];
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			q[col + NCB - 1] = r[col + NCB - 1]*r[col + NCB - 1];
			const double d = wv[col]*wv[col];
			SRH_SCHED_BARRIER();
#pragma unroll
			for (int j = 0; j < NCB; ++j) P[j] = __builtin_fma(wv[col], r[col + j], P[j]);
#pragma unroll
			for (int j = 0; j < NCB; ++j) Q[j] = __builtin_fma(cv[col], r[col + j], Q[j]);
#pragma unroll
			for (int j = 0; j < NCB; ++j) U[j] = __builtin_fma(d, q[col + j], U[j]);
			SRH_SCHED_BARRIER();
			if (col & 1) {
				next.r2(col >> 1, r[col - 1], r[col]);
				next.w2(col >> 1, wv[col - 1], wv[col]);
				next.c2(col >> 1, cv[col - 1], cv[col]);
			}
			SRH_SCHED_BARRIER();
		}
#pragma unroll
		for (int m = (WS - 1)/2; m < NR/2; ++m) next.r2(m, r[2*m], r[2*m + 1]);
		wv[WS - 1] = next.w(WS - 1);
		cv[WS - 1] = next.c(WS - 1);
		src.row_end(seen);
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { Pout[j] = P[j]; Qout[j] = Q[j]; Uout[j] = U[j]; }
}

// ---- the finishes ---------------------------------------------------------------------------------------------------------
// twoviewstereo.cpp:976 before the clamp; s2 = the pixel's sum2
SRH_NHD double two_sweep_finish(double s1, double s2, double s3) { return 255*(1.0 - fabs(s1) / sqrt(s2 * s3)); }

// the seed of 1/sqrt(x): v_rsq_f64 on the device.  onepass_finish trusts it for nothing
SRH_NHD double rsq_seed(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_rsq(x);
#else
	return 1.0/sqrt(x);
#endif
}

// The finish of a one-pass candidate: the sums recovered from P, Q, U, the cost without an IEEE division or square root,
// and the certificate (srh_wta.hpp has the derivation).  itw = fl(1/totalWeight) (pconst slot 3), TT = T, SA = the pixel's
// sum of fma(w, l, -meanL).  A non-positive or NaN sum3 gives a NaN residual and fails the certificate; an uncertified
// value is never used.
SRH_NHD double onepass_finish(double P, double Q, double U, double SA, double itw, double s2, double TT,
                              double sig3, double zmax2, bool &okc)
{
	const double m = P*itw, p2 = P + P;
	const double s3 = __builtin_fma(-m, __builtin_fma(-TT, m, p2), U);    // U - m*(2P - T*m)
	const double s1 = __builtin_fma(-m, SA, Q);
	const double q3 = __builtin_fma(m, __builtin_fma(TT, m, p2), U);      // U + m*(2P + T*m)
	const double x = s2*s3;
	const double y0 = rsq_seed(x);
	const double e = __builtin_fma(-(x*y0), y0, 1.0);                     // 1 - x*y0^2
	const double y1 = __builtin_fma(y0*e, __builtin_fma(0.375, e, 0.5), y0);
	const bool c1 = s3 >= sig3, c2 = s3*zmax2 >= q3, c3 = __builtin_fabs(e) <= 0x1p-20;
	okc = c1 & c2 & c3;                                                   // (no short circuit: three compares, no branch)
	return __builtin_fma(-255.0, __builtin_fabs(s1)*y1, 255.0);
}

// What a cost kernel stores for a fast-form candidate of value v.  Exact forms (CERT = false): the reference's clamp
// (twoviewstereo.cpp:976).  Certified forms: NaN for a candidate the bound does not cover (certified = false: sum3 below
// sigma3, resp. the one-pass certificate), the clamp for a value above clamp + e0 (m_hi; the clamp is 1-Lipschitz, so the
// reference's value is the clamp), else the value AS IT IS -- also when its own bits are the clamp's or it lies in
// (clamp, clamp + e0]: the clamp gap of srh_wta.hpp's table.
// B = const double &: the bounds are read where the rule needs them, as in the expression written out on a kernel's arguments
// (the two-sweep sites; by value the compiler turns the rule into selects, and their register allocation moves).
template <bool CERT, class B = double>
SRH_NHD double block_stored(double v, bool certified, B m_hi, B clamp)
{
	if (CERT) return !certified ? __builtin_nan("") : (v > m_hi ? clamp : v);
	return (v < clamp) ? v : clamp;
}

}  // namespace srh
