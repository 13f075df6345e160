// srh_labels.hpp -- the label axis of a [pixel][label] volume across one wave: what srh_twoview_mrf.hip (TRW-S) and
// srh_twoview_sgm.hip (semi-global aggregation) share.  A pixel's L <= 256 labels lie across the 64 lanes of a wave,
// NL = ceil(L/64) <= 4 consecutive labels per lane (label = lane*NL + j); a lane holds +inf on labels that do not exist.
//   wave_min / wave_argmin   wave-wide reductions by DPP, the result in every lane
//   trunc_message            the truncated-linear message  M[k] = min_ks (buf[ks] + lambda*min(|k - ks|, smooth_max))  in its
//                            window form (the head of srh_twoview_mrf.hip says why these are the bits of the direct form)
//   load_pieces / store_pieces   a lane's NL labels 16 bytes at a time
#pragma once
#include <hip/hip_runtime.h>

namespace srh {

namespace {

typedef unsigned long long u64;

// Wave-wide reductions by DPP (no LDS round trips in the step's dependent chain): row_shr 1, 2, 4, 8 leave a row's result
// in its lane 15 (min is idempotent: the overlapping spans do no harm), row_bcast:15 into rows 1 and 3 and row_bcast:31 into
// rows 2 and 3 leave the wave's in lane 63, which every lane then reads.  A lane without a source keeps its own value.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_keep(double v) {
	return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_keep(int v) {
	return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ double read_lane63(double v) {
	const long long b = __double_as_longlong(v);
	const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), 63);
	return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
#define TM_DPP_STEPS(F) F(0x111, 0xf) F(0x112, 0xf) F(0x114, 0xf) F(0x118, 0xf) F(0x142, 0xa) F(0x143, 0xc)
// the smallest of the wave's 64 values, in every lane
__device__ __forceinline__ double wave_min(double v) {
#define TM_MIN_STEP(CTRL, RM) { const double t = dpp_keep<CTRL, RM>(v); v = v > t ? t : v; }
	TM_DPP_STEPS(TM_MIN_STEP)
#undef TM_MIN_STEP
	return read_lane63(v);
}
// the smallest value and, among equal ones, the lowest index
__device__ __forceinline__ void wave_argmin(double &v, int &i) {
#define TM_ARG_STEP(CTRL, RM) { const double t = dpp_keep<CTRL, RM>(v); const int ti = dpp_keep<CTRL, RM>(i); \
	                            if (v > t || (v == t && ti < i)) { v = t; i = ti; } }
	TM_DPP_STEPS(TM_ARG_STEP)
#undef TM_ARG_STEP
	v = read_lane63(v);
	i = __builtin_amdgcn_readlane(i, 63);
}

// the truncated-linear message of buf (a lane's labels lane*NL .. lane*NL + NL - 1; +inf on labels that do not exist):
// c[d] = lambda*d, cmax = lambda*smooth_max, nwin = the largest d < smooth_max
template <int NL>
__device__ __forceinline__ void trunc_message(const double (&buf)[NL], int lane, int nwin, const double (&c)[4], double cmax, double (&M)[NL])
{
	const double inf = __builtin_inf();
	double ext[NL + 6];                                          // labels lane*NL - 3 .. lane*NL + NL + 2
#pragma unroll
	for (int j = 0; j < NL; ++j) ext[3 + j] = buf[j];
#pragma unroll
	for (int k = 1; k <= 3; ++k) {
		{	// label lane*NL - k = (lane - off)*NL + jj
			const int off = (k + NL - 1)/NL, jj = off*NL - k;
			const double t = __shfl(buf[jj], (lane - off) & 63);
			ext[3 - k] = lane >= off ? t : inf;
		}
		{	// label lane*NL + NL - 1 + k = (lane + off)*NL + jj
			const int idx = NL - 1 + k, off = idx/NL, jj = idx % NL;
			const double t = __shfl(buf[jj], (lane + off) & 63);
			ext[3 + NL - 1 + k] = lane + off < 64 ? t : inf;
		}
	}
	double g = buf[0];
#pragma unroll
	for (int j = 1; j < NL; ++j) g = g > buf[j] ? buf[j] : g;
	g = wave_min(g);
	const double gm = g + cmax;
#pragma unroll
	for (int j = 0; j < NL; ++j) {
		double m = ext[3 + j] + c[0];
#pragma unroll
		for (int d = 1; d <= 3; ++d) {
			if (d <= nwin) {
				const double t1 = ext[3 + j - d] + c[d], t2 = ext[3 + j + d] + c[d];
				m = m > t1 ? t1 : m;
				m = m > t2 ? t2 : m;
			}
		}
		M[j] = m > gm ? gm : m;
	}
}

// a lane's NL consecutive labels as 16-byte pieces (NL even, L a multiple of NL: the lane's labels exist or do not together,
// and its piece of every [pixel][L] row starts on an even double)
template <int NL> __device__ __forceinline__ void load_pieces(const double *p, bool c, double (&o)[NL]) {
#pragma unroll
	for (int j = 0; j < NL; j += 2) {
		double2 v = make_double2(0.0, 0.0);
		if (c) v = *reinterpret_cast<const double2 *>(p + j);
		o[j] = v.x; o[j + 1] = v.y;
	}
}
template <int NL> __device__ __forceinline__ void store_pieces(double *p, const double (&v)[NL]) {
#pragma unroll
	for (int j = 0; j < NL; j += 2) *reinterpret_cast<double2 *>(p + j) = make_double2(v[j], v[j + 1]);
}

} // namespace

} // namespace srh
