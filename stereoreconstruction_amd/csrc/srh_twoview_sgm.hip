// srh_twoview_sgm.hip -- semi-global aggregation over TwoViewStereo's label cost volume.  NOT IN THE
// REFERENCE: a second, non-iterative minimiser of the MRF stage's energy (srh_twoview_mrf.hip), between the
// winner-take-all and TRW-S.  The definition (include/stereo_recon_hip.h states it in full): for each enabled direction r
// of (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (+1,-1) (-1,+1), along every path line,
//     L_r(p, .) = C(p, .)                                       where p - r is outside the image,
//     L_r(p, d) = C(p, d) + (M[d] - g)                          otherwise, with prev = L_r(p - r, .), g = min prev and
//     M[d] = min( min_{|j| < smooth_max} (prev[d + j] + lambda*|j|),  g + lambda*smooth_max )
// -- the truncated-linear message of srh_labels.hpp, the very code of the TRW-S pass.  S = the sum of the L_r in ascending
// direction index, label = the lowest argmin of S, depth = depthFromLabel(label) where the mask is WHITE.
//
// The path kernel: ONE WAVE PER PATH LINE (a row, a column, a diagonal), the labels across its 64 lanes as in the TRW-S pass
// kernel, prev in registers along the line.  The data costs (and, from the second direction on, the sums) of the next
// SG_AHEAD pixels of the line are in flight while a pixel is computed: those loads do not depend on the chain.  One launch
// per direction; every S entry is touched by exactly one wave of a launch, so there are no atomics, no hand-overs between
// workgroups and no waits: every loop is bounded by the line's length.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_labels.hpp"

namespace srh {

namespace {

constexpr int SG_WAVES = 4;             // path lines per workgroup (the waves share nothing)
constexpr int SG_AHEAD = 4;             // pixels of a line whose loads are in flight

struct SgmPathArgs {
	int W, H, L, nwin;
	int dx, dy, nlines;
	double cmax, c[4];
	const double *C;                    // [n][L] data costs
	double *S;                          // [n][L] sums
};

// FIRST: the first enabled direction writes S, the later ones add to it
// VEC: L is a multiple of NL, NL is even and both volumes start on a 16-byte boundary
template <int NL, bool VEC, bool FIRST>
__global__ __launch_bounds__(SG_WAVES*64) void twoview_sgm_path_kernel(const SgmPathArgs a)
{
	const int lane = threadIdx.x & 63;
	const int line = blockIdx.x*SG_WAVES + (threadIdx.x >> 6);      // wave-uniform
	if (line >= a.nlines) return;
	const int W = a.W, H = a.H, L = a.L, dx = a.dx, dy = a.dy;
	// the line's first pixel (the one whose predecessor is outside) and its length
	int x0, y0;
	if (dy == 0) { x0 = dx > 0 ? 0 : W - 1; y0 = line; }
	else if (dx == 0) { x0 = line; y0 = dy > 0 ? 0 : H - 1; }
	else if (line < W) { x0 = line; y0 = dy > 0 ? 0 : H - 1; }
	else { x0 = dx > 0 ? 0 : W - 1; y0 = dy > 0 ? line - W + 1 : H - 1 - (line - W + 1); }
	int len = W + H;
	if (dx != 0) len = min(len, dx > 0 ? W - x0 : x0 + 1);
	if (dy != 0) len = min(len, dy > 0 ? H - y0 : y0 + 1);
	const long n0 = (long)y0*W + x0, dn = (long)dy*W + dx;          // pixel index of step s: n0 + s*dn
	const double inf = __builtin_inf();
	const int nwin = a.nwin;
	const double cmax = a.cmax;
	const double cc[4] = { a.c[0], a.c[1], a.c[2], a.c[3] };
	bool lv[NL];
#pragma unroll
	for (int j = 0; j < NL; ++j) lv[j] = lane*NL + j < L;

	double ringC[SG_AHEAD][NL], ringS[SG_AHEAD][NL];
	auto fetch = [&](int s, double (&oc)[NL], double (&os)[NL]) {
		const long at = (n0 + (long)s*dn)*L + lane*NL;
		if (VEC) {
			load_pieces<NL>(a.C + at, lv[0], oc);
			if (!FIRST) load_pieces<NL>(a.S + at, lv[0], os);
		} else {
#pragma unroll
			for (int j = 0; j < NL; ++j) {
				oc[j] = lv[j] ? a.C[at + j] : 0.0;
				if (!FIRST) os[j] = lv[j] ? a.S[at + j] : 0.0;
			}
		}
	};
#pragma unroll
	for (int k = 0; k < SG_AHEAD; ++k) {
#pragma unroll
		for (int j = 0; j < NL; ++j) { ringC[k][j] = 0.0; ringS[k][j] = 0.0; }
		if (k < len) fetch(k, ringC[k], ringS[k]);
	}

	double prev[NL];
#pragma unroll
	for (int j = 0; j < NL; ++j) prev[j] = inf;
	for (int s0 = 0; s0 < len; s0 += SG_AHEAD) {
#pragma unroll
		for (int k = 0; k < SG_AHEAD; ++k) {
			const int s = s0 + k;
			if (s < len) {                                              // (wave-uniform)
				double Cv[NL], Sv[NL], Lr[NL];
#pragma unroll
				for (int j = 0; j < NL; ++j) { Cv[j] = ringC[k][j]; Sv[j] = ringS[k][j]; }
				if (s + SG_AHEAD < len) fetch(s + SG_AHEAD, ringC[k], ringS[k]);
				if (s == 0) {
#pragma unroll
					for (int j = 0; j < NL; ++j) Lr[j] = Cv[j];
				} else {
					double M[NL], g = prev[0];
#pragma unroll
					for (int j = 1; j < NL; ++j) g = g > prev[j] ? prev[j] : g;
					g = wave_min(g);                                        // (trunc_message's own: one chain after CSE)
					trunc_message<NL>(prev, lane, nwin, cc, cmax, M);
#pragma unroll
					for (int j = 0; j < NL; ++j) { const double t = M[j] - g; Lr[j] = Cv[j] + t; }
				}
				double out[NL];
#pragma unroll
				for (int j = 0; j < NL; ++j) {
					prev[j] = lv[j] ? Lr[j] : inf;
					out[j] = FIRST ? Lr[j] : Sv[j] + Lr[j];
				}
				const long at = (n0 + (long)s*dn)*L + lane*NL;
				if (VEC) { if (lv[0]) store_pieces<NL>(a.S + at, out); }
				else {
#pragma unroll
					for (int j = 0; j < NL; ++j) if (lv[j]) a.S[at + j] = out[j];
				}
			}
		}
	}
}

// label = the lowest argmin of a pixel's sums (a wave per pixel), depth = depthFromLabel(label) where the mask is WHITE
// (twoviewstereo.cpp:324), NaN elsewhere
template <int NL>
__global__ __launch_bounds__(SG_WAVES*64) void twoview_sgm_readoff_kernel(const ViewDev *__restrict__ views, int slot, srh_params P, int L,
                                                                          const double *__restrict__ S, int32_t *__restrict__ ans)
{
	const ViewDev &V = views[slot];
	const int lane = threadIdx.x & 63;
	const long n = (long)blockIdx.x*SG_WAVES + (threadIdx.x >> 6);  // wave-uniform
	if (n >= (long)V.w*V.h) return;
	double best = __builtin_inf();
	int lab = 0x7fffffff;
#pragma unroll
	for (int j = 0; j < NL; ++j) {
		const int k = lane*NL + j;
		if (k < L) {
			const double v = S[n*L + k];
			if (lab == 0x7fffffff || best > v) { best = v; lab = k; }
		}
	}
	wave_argmin(best, lab);
	if (lane == 0) {
		ans[n] = lab;
		V.depth[n] = V.mask[n] == 1 ? depth_from_label(P, false, lab) : __builtin_nan("");
	}
}

template <int NL, bool VEC> static hipError_t launch_path_nl(hipStream_t st, const SgmPathArgs &a, bool first)
{
	const dim3 grid((unsigned)((a.nlines + SG_WAVES - 1)/SG_WAVES)), block(SG_WAVES*64);
	if (first) hipLaunchKernelGGL((twoview_sgm_path_kernel<NL, VEC, true>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((twoview_sgm_path_kernel<NL, VEC, false>), grid, block, 0, st, a);
	return hipGetLastError();
}

const int sgm_dirs[8][2] = { { 1, 0 }, { -1, 0 }, { 0, 1 }, { 0, -1 }, { 1, 1 }, { -1, -1 }, { 1, -1 }, { -1, 1 } };

} // namespace

void twoview_sgm_layout(double *buf, int w, int h, int L, TvSgmLayout &lay)
{
	const size_t n = (size_t)w*h;
	const size_t vol = (n*(size_t)L + 1) & ~(size_t)1;                 // every block starts 16-byte aligned
	lay.S = buf;
	lay.partial = buf + vol;
	lay.nparts = (int)((n + 255)/256);
	lay.energy = lay.partial + ((lay.nparts + 1) & ~1);                // [0] energy, [1] unused
	lay.ans = reinterpret_cast<int32_t *>(lay.energy + 2);
	lay.total_doubles = vol + ((lay.nparts + 1) & ~1) + 2 + (n + 1)/2;
}

size_t twoview_sgm_scratch_doubles(int w, int h, int L)
{
	TvSgmLayout lay;
	twoview_sgm_layout(nullptr, w, h, L, lay);
	return lay.total_doubles;
}

// direction k of the fixed list: L_k along every line, written to S (first) or added to it
hipError_t launch_twoview_sgm_path(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax, int k, bool first)
{
	TvSgmLayout lay;
	twoview_sgm_layout(buf, w, h, L, lay);
	SgmPathArgs a;
	a.W = w; a.H = h; a.L = L;
	a.dx = sgm_dirs[k][0]; a.dy = sgm_dirs[k][1];
	a.nlines = a.dy == 0 ? h : a.dx == 0 ? w : w + h - 1;
	a.cmax = lambda*smax;
	for (int d = 0; d < 4; ++d) a.c[d] = lambda*(double)d;
	a.nwin = 0;
	while (a.nwin < 3 && (double)(a.nwin + 1) < smax) ++a.nwin;        // the largest d < smooth_max
	a.C = costs; a.S = lay.S;
	// the 16-byte form needs both volumes on a 16-byte boundary (the scratch buffer's is; launch_pass's rule)
	const bool vec = ((reinterpret_cast<uintptr_t>(a.C) | reinterpret_cast<uintptr_t>(a.S)) & 15) == 0;
	switch ((L + 63)/64) {
	case 1: return launch_path_nl<1, false>(st, a, first);
	case 2: return vec && L % 2 == 0 ? launch_path_nl<2, true>(st, a, first) : launch_path_nl<2, false>(st, a, first);
	case 3: return launch_path_nl<3, false>(st, a, first);
	default: return vec && L % 4 == 0 ? launch_path_nl<4, true>(st, a, first) : launch_path_nl<4, false>(st, a, first);
	}
}

hipError_t launch_twoview_sgm_readoff(hipStream_t st, const ViewDev *views, int slot, const srh_params &P, double *buf, int w, int h, int L)
{
	TvSgmLayout lay;
	twoview_sgm_layout(buf, w, h, L, lay);
	const size_t n = (size_t)w*h;
	const dim3 grid((unsigned)((n + SG_WAVES - 1)/SG_WAVES)), block(SG_WAVES*64);
	switch ((L + 63)/64) {
	case 1: hipLaunchKernelGGL(twoview_sgm_readoff_kernel<1>, grid, block, 0, st, views, slot, P, L, lay.S, lay.ans); break;
	case 2: hipLaunchKernelGGL(twoview_sgm_readoff_kernel<2>, grid, block, 0, st, views, slot, P, L, lay.S, lay.ans); break;
	case 3: hipLaunchKernelGGL(twoview_sgm_readoff_kernel<3>, grid, block, 0, st, views, slot, P, L, lay.S, lay.ans); break;
	default: hipLaunchKernelGGL(twoview_sgm_readoff_kernel<4>, grid, block, 0, st, views, slot, P, L, lay.S, lay.ans); break;
	}
	return hipGetLastError();
}

// E(label) under the MRF stage's energy, by its kernels, into lay.energy[0]
hipError_t launch_twoview_sgm_energy(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax)
{
	TvSgmLayout lay;
	twoview_sgm_layout(buf, w, h, L, lay);
	return launch_twoview_labels_energy(st, costs, lay.ans, lay.partial, lay.nparts, lay.energy, w, h, L, lambda, smax);
}

} // namespace srh
