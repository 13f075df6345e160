// srh_mvs_sgm.hip -- semi-global aggregation over MultiViewStereo's top-K peak labels.  NOT IN THE
// REFERENCE: a second, non-iterative minimiser of the MRF branch's energy (srh_mrf.hip), between "best peak wins" and
// TRW-S.  The definition (include/stereo_recon_hip.h states it in full): labels 0 .. K-1 are a pixel's peaks, K is
// "unknown"; D and V are the MRF branch's dataCost and smoothnessCost; for each enabled direction r of (+1,0) (-1,0) (0,+1)
// (0,-1) (+1,+1) (-1,-1) (+1,-1) (-1,+1), along every path line, with q = p - r,
//     L_r(p, .) = D(p, .)                                       where q is outside the image,
//     L_r(p, d) = D(p, d) + (M[d] - g)                          otherwise, with prev = L_r(q, .), g = min_k prev[k] and
//     M[d] = min_k (prev[k] + V(q, k; p, d))
// S = the sum of the L_r in ascending direction index, label = the lowest argmin of S, depth = the chosen peak's where the
// mask is WHITE.
//
// Unlike TwoViewStereo's aggregation (srh_twoview_sgm.hip) the pairwise term is no function of a label distance: between
// two peaks it is 2|zq - zp|/(zq + zp) of the two pixels' own depths, so the message is a dense (K+1) x (K+1) min-plus
// product whose matrix changes at every edge, every entry an IEEE division.
//
// The path kernel: the label layout of the TRW-S pass -- 16 lanes per pixel, lane = destination label d, rows of 16 doubles
// in D / pz / S -- so a wave carries FOUR path lines (rows, columns or diagonals), and a line belongs to exactly one wave.
// prev and the predecessor's depths stay in the line's 16 lanes; prev[k] and zq[k] reach lane d by DPP row broadcasts.  A
// line's data costs, depths and (from the second direction on) sums are fetched a chunk of MS_CH pixels ahead, and a chunk's
// results are stored after its last step.  The K quotients of a step depend on the two pixels' depths alone, not on the
// chain: the column V(., k; next pixel, d) is evaluated during the current step, so that what a step has to wait for is K + 1
// adds and a minimum, not divisions.  One launch per direction; every S entry is touched by exactly one wave of a launch, so
// there are no atomics, no hand-overs between workgroups and no waits: every loop is bounded by the line's length.
#include "srh_internal.hpp"
#include "srh_peaks.hpp"

#include <type_traits>

namespace srh {

namespace {

constexpr int MS_WAVES = 4;             // waves per workgroup (they share nothing)
constexpr int MS_LINES = 4;             // path lines per wave: 16 lanes each
constexpr int MS_CH = 4;                // pixels of a line per fetched chunk

// runs f once per label I = 0 .. N-1, I a compile-time constant (a DPP lane select is an immediate)
template <int I, int N, class F> __device__ __forceinline__ void for_labels(F &&f) {
	if constexpr (I < N) { f(std::integral_constant<int, I>()); for_labels<I + 1, N>(f); }
}

// bc16 and a rotation within a pixel's 16 lanes where all of them are active (the path kernel's step has no divergent
// branch): every lane has a source, so bound_ctrl changes no value and spares the destination's initialisation
template <int I> __device__ __forceinline__ double row_bc(double v) {
	return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + I, 0xf, 0xf, true);       // row_newbcast:I
}
template <int N> __device__ __forceinline__ double row_ror(double v) {
	return __builtin_amdgcn_update_dpp(0.0, v, 0x120 + N, 0xf, 0xf, true);       // row_ror:N
}
// the smallest of a pixel's 16 values, in each of its lanes (no NaN, no negative zero among them: any order, the same bits)
__device__ __forceinline__ double row_min(double v) {
	v = __builtin_fmin(v, row_ror<8>(v));
	v = __builtin_fmin(v, row_ror<4>(v));
	v = __builtin_fmin(v, row_ror<2>(v));
	return __builtin_fmin(v, row_ror<1>(v));
}

struct MvsSgmPathArgs {
	int W, H, K;
	int dx, dy, nlines;
	double psi, psi2;
	const double *D;                    // [n][16] data costs
	const double *pz;                   // [n][16] peak depths (label K and above: 0)
	double *S;                          // [n][16] sums
};

struct MsChunk { double D[MS_CH], Z[MS_CH], S[MS_CH]; };

// FIRST: the first enabled direction writes S, the later ones add to it
// LT: the label count K + 1 when known at compile time (10 for the reference's K = 9: straight-line label loops), 0: any
template <int LT, bool FIRST>
__global__ __launch_bounds__(MS_WAVES*64) void mvs_sgm_path_kernel(const MvsSgmPathArgs a)
{
	constexpr int NL = LT ? LT : 16;
	const int d = threadIdx.x & 15;
	const int line = (int)blockIdx.x*(MS_WAVES*MS_LINES) + (int)(threadIdx.x >> 4);   // the same in a pixel's 16 lanes
	const int W = a.W, H = a.H, K = LT ? LT - 1 : a.K, L = K + 1, dx = a.dx, dy = a.dy;
	const double psi = a.psi, psi2 = a.psi2;
	// the line's first pixel (the one whose predecessor is outside) and its length; no line: length 0
	int x0 = 0, y0 = 0, len = 0;
	if (line < a.nlines) {
		if (dy == 0) { x0 = dx > 0 ? 0 : W - 1; y0 = line; }
		else if (dx == 0) { x0 = line; y0 = dy > 0 ? 0 : H - 1; }
		else if (line < W) { x0 = line; y0 = dy > 0 ? 0 : H - 1; }
		else { x0 = dx > 0 ? 0 : W - 1; y0 = dy > 0 ? line - W + 1 : H - 1 - (line - W + 1); }
		len = W + H;
		if (dx != 0) len = min(len, dx > 0 ? W - x0 : x0 + 1);
		if (dy != 0) len = min(len, dy > 0 ? H - y0 : y0 + 1);
	}
	const long n0 = (long)y0*W + x0, dn = (long)dy*W + dx;          // pixel index of step s: n0 + s*dn
	const bool lv = d < L, unknown = d == K;
	const double vu = unknown ? 0.0 : psi;                          // V(q, "unknown"; p, d)

	auto load_chunk = [&](int c, MsChunk &B) {
#pragma unroll
		for (int j = 0; j < MS_CH; ++j) {
			const int s = c*MS_CH + j;
			const bool ok = s < len;
			const long at = (n0 + (long)s*dn)*16 + d;
			B.D[j] = ok ? a.D[at] : 0.0;
			B.Z[j] = ok ? a.pz[at] : 1.0;
			B.S[j] = (!FIRST && ok && lv) ? a.S[at] : 0.0;
		}
	};

	MsChunk cur, nxt;
	load_chunk(0, nxt);
	double prev = 0.0, g = 0.0;                                     // L_r of the line's previous pixel, this lane's label; its minimum
	double V[16];                                                   // V(q, k; p, d) of the step to come, k = 0 .. K
#pragma unroll
	for (int k = 0; k < 16; ++k) V[k] = vu;

	// (the bound is the longest of the wave's four lines; a shorter line's lanes go on computing on padding and store nothing)
	for (int c = 0; __any(c*MS_CH < len); ++c) {
		cur = nxt;
		load_chunk(c + 1, nxt);
		double out[MS_CH];
#pragma unroll
		for (int j = 0; j < MS_CH; ++j) {
			const int s = c*MS_CH + j;
			// the dependent chain: K + 1 broadcasts and adds and a minimum, then the minimum of the result over its labels
			double M = 0.0;
			for_labels<0, NL>([&](auto ic) {
				constexpr int KS = decltype(ic)::value;
				if (!LT && KS >= L) return;                             // (wave-uniform)
				const double t = row_bc<KS>(prev) + V[KS];
				M = KS == 0 ? t : __builtin_fmin(M, t);
			});
			const double m = M - g;
			const double Lr = s == 0 ? cur.D[j] : cur.D[j] + m;
			prev = Lr;
			g = row_min(lv ? Lr : __builtin_inf());
			out[j] = FIRST ? Lr : cur.S[j] + Lr;
			// off the chain: the next step's column of V, from this pixel's depths (broadcast) and the next pixel's (own lane)
			const double zp = cur.Z[j], zn = j + 1 < MS_CH ? cur.Z[(j + 1) % MS_CH] : nxt.Z[0];
			for_labels<0, NL - 1>([&](auto ic) {
				constexpr int KS = decltype(ic)::value;
				if (!LT && KS >= K) return;
				V[KS] = smooth_peak(row_bc<KS>(zp), zn, unknown, psi, psi2);
			});
		}
#pragma unroll
		for (int j = 0; j < MS_CH; ++j) {
			const int s = c*MS_CH + j;
			if (s < len && lv) a.S[(n0 + (long)s*dn)*16 + d] = out[j];
		}
	}
}

// label = the lowest argmin of a pixel's sums, 16 lanes per pixel
__global__ __launch_bounds__(256) void mvs_sgm_readoff_kernel(long n, int K, const double *__restrict__ S, int32_t *__restrict__ ans)
{
	const int d = threadIdx.x & 15, L = K + 1;
	const long p = (long)blockIdx.x*16 + (threadIdx.x >> 4);
	const bool ok = p < n;
	const double v = (ok && d < L) ? S[p*16 + d] : __builtin_inf();
	double best = 0.0;
	int lab = 0;
	for_labels<0, 16>([&](auto ic) {
		constexpr int KS = decltype(ic)::value;
		if (KS >= L) return;
		const double t = bc16<KS>(v);
		if (KS == 0 || best > t) { best = t; lab = KS; }
	});
	if (ok && d == 0) ans[p] = lab;
}

template <int LT> hipError_t launch_path_lt(hipStream_t st, const MvsSgmPathArgs &a, bool first)
{
	constexpr int per = MS_WAVES*MS_LINES;
	const dim3 grid((unsigned)((a.nlines + per - 1)/per)), block(MS_WAVES*64);
	if (first) hipLaunchKernelGGL((mvs_sgm_path_kernel<LT, true>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((mvs_sgm_path_kernel<LT, false>), grid, block, 0, st, a);
	return hipGetLastError();
}

const int sgm_dirs[8][2] = { { 1, 0 }, { -1, 0 }, { 0, 1 }, { 0, -1 }, { 1, 1 }, { -1, -1 }, { 1, -1 }, { -1, 1 } };

} // namespace

void mvs_sgm_layout(double *buf, int w, int h, MvsSgmLayout &lay)
{
	const size_t n = (size_t)w*h;
	lay.pz = buf; lay.D = buf + n*16; lay.S = buf + n*32;
	lay.partial = buf + n*48;
	lay.nparts = (int)((n + 255)/256);
	lay.energy = lay.partial + ((lay.nparts + 1) & ~1);                // [0] energy, [1] unused
	lay.ans = reinterpret_cast<int32_t *>(lay.energy + 2);
	lay.total_doubles = n*48 + ((lay.nparts + 1) & ~1) + 2 + (n + 1)/2;
}

size_t mvs_sgm_scratch_doubles(int w, int h)
{
	MvsSgmLayout lay;
	mvs_sgm_layout(nullptr, w, h, lay);
	return lay.total_doubles;
}

// D and pz of every pixel, by the MRF branch's data kernel
hipError_t launch_mvs_sgm_setup(hipStream_t st, double *buf, int w, int h, int K, double beta, double lambda, double phiu, const double *peaks)
{
	MvsSgmLayout lay;
	mvs_sgm_layout(buf, w, h, lay);
	return launch_mrf_data(st, (size_t)w*h, K, beta, lambda, phiu, peaks, lay.D, lay.pz);
}

// direction k of the fixed list: L_k along every line, written to S (first) or added to it
hipError_t launch_mvs_sgm_path(hipStream_t st, double *buf, int w, int h, int K, double psiu, int k, bool first)
{
	MvsSgmLayout lay;
	mvs_sgm_layout(buf, w, h, lay);
	MvsSgmPathArgs a;
	a.W = w; a.H = h; a.K = K;
	a.dx = sgm_dirs[k][0]; a.dy = sgm_dirs[k][1];
	a.nlines = a.dy == 0 ? h : a.dx == 0 ? w : w + h - 1;
	a.psi = psiu; a.psi2 = 2*psiu;
	a.D = lay.D; a.pz = lay.pz; a.S = lay.S;
	return K == 9 ? launch_path_lt<10>(st, a, first) : launch_path_lt<0>(st, a, first);
}

// labels from the sums, then the depth map by the MRF branch's rule
hipError_t launch_mvs_sgm_readoff(hipStream_t st, const ViewDev *views, int slot, double *buf, int w, int h, int K)
{
	MvsSgmLayout lay;
	mvs_sgm_layout(buf, w, h, lay);
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(mvs_sgm_readoff_kernel, dim3((unsigned)((n + 15)/16)), dim3(256), 0, st, (long)n, K, lay.S, lay.ans);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	return launch_mrf_labels_depth(st, views, slot, K, lay.pz, lay.ans, n);
}

// totalEnergy() of the labels under the MRF branch's energy, by its kernels, into lay.energy[0]
hipError_t launch_mvs_sgm_energy(hipStream_t st, double *buf, int w, int h, int K, double psiu)
{
	MvsSgmLayout lay;
	mvs_sgm_layout(buf, w, h, lay);
	return launch_mrf_labels_energy(st, w, h, K, psiu, lay.D, lay.pz, lay.ans, lay.partial, lay.nparts, lay.energy);
}

} // namespace srh
