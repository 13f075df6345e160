// srh_mvs_subpixel.hip -- sub-pixel depth for a MultiViewStereo view's finished depth map (srh_mvs_view_subpixel).
//
// A view's depth is the best of the top-K peaks over its neighbours, or a peak picked afterwards by TRW-S or the semi-global
// stage: no estimator keeps the (neighbour, pixel) that gave it.  The map identifies it: exactly one (neighbour, curve pixel)
// has candidate_depth equal to the stored depth bit for bit.  Per pixel (x, y) of the view, z0 its depth:
//
//   1. outside the mask, z0 not finite or z0 <= 0 (NaN, +INF, the "no peak" value -1): NONE.
//   2. the winner: for the neighbours in the order given, for q in the order of walk_curve<true>, the first (i, q) with
//      candidate_depth(q) == z0.  None: NO_WINNER.
//   3. S = the pixels of the winner's curve, A = the members of S at Chebyshev distance 1 from the winner; n- and n+ as in
//      srh_subpixel.hip (ascending (qy, qx), strict comparisons).  One missing: NO_NEIGHBOUR.
//   4. c-, c0, c+ = mvs_cost (higher is better) of the pixel against n-, the winner, n+; the class and delta are those of
//      srh_subpixel.hip on (-c-, -c0, -c+); the new depth is candidate_depth at winner + |delta|*(n - winner).
//
// Two kernels.  mvs_subpixel_search_kernel (one lane per pixel) finds the winner and its neighbours.  Its default form
// triangulates only the curve pixels within SRH_MVSSUB_RADIUS of the pixel that holds the projection of the reference
// pixel's point at z0 -- and keeps, in the same walk, a 9 x 9 bit map of the visited pixels there, from which the winner's
// adjacency is read; a pixel with no winner there takes the exhaustive form: every curve pixel of every neighbour, then a
// second walk of the winner's curve with the AdjacencyVisitor.  mvs_subpixel_refine_kernel: one workgroup of 128 lanes per
// 32-pixel window tile, lanes 0-31 take n-, 32-63 the winner, 64-95 n+; the costs meet in LDS and lanes 0-31 finish.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_depth_at.hpp"
#include "srh_mvs_subpixel.hpp"

namespace srh {

// exhaustive search: the first visited pixel whose candidate_depth is z0
struct MvsWinnerVisitor {
	const srh_camera &A, &B;
	const srh_params &P;
	const Ray &ray;
	double z0;
	int wx, wy;
	bool found;
	__device__ __forceinline__ void operator()(int cx, int cy) {
		if (found) return;
		if (candidate_depth(A, B, P, ray, cx, cy) == z0) { found = true; wx = cx; wy = cy; }
	}
};

// narrowed search: the same among the pixels within SRH_MVSSUB_RADIUS of (px, py); every visited pixel within one more
// sets bit (dy + NR)*NW + (dx + NR) of (lo, hi) -- a pixel seen before cannot match now and is not triangulated again
struct MvsNarrowVisitor {
	static constexpr int NR = SRH_MVSSUB_RADIUS + 1, NW = 2*NR + 1;
	static_assert(NW*NW <= 128, "the visited map is two 64-bit words");
	const srh_camera &A, &B;
	const srh_params &P;
	const Ray &ray;
	double z0;
	int px, py;
	int wx, wy;
	bool found;
	unsigned long long lo, hi;
	__device__ __forceinline__ bool bit(int dx, int dy) const {
		const int b = (dy + NR)*NW + (dx + NR);
		return ((b < 64 ? lo >> b : hi >> (b - 64)) & 1ull) != 0;
	}
	__device__ __forceinline__ void operator()(int cx, int cy) {
		const int dx = cx - px, dy = cy - py;
		if (dx < -NR || dx > NR || dy < -NR || dy > NR) return;
		const bool seen = bit(dx, dy);
		const int b = (dy + NR)*NW + (dx + NR);
		if (b < 64) lo |= 1ull << b; else hi |= 1ull << (b - 64);
		if (found || seen || dx < -SRH_MVSSUB_RADIUS || dx > SRH_MVSSUB_RADIUS || dy < -SRH_MVSSUB_RADIUS || dy > SRH_MVSSUB_RADIUS) return;
		if (candidate_depth(A, B, P, ray, cx, cy) == z0) { found = true; wx = cx; wy = cy; }
	}
	// the AdjacencyVisitor's mask around the winner
	__device__ __forceinline__ unsigned adjacency() const {
		unsigned m = 0;
#pragma unroll
		for (int k = 0; k < 9; ++k) {
			const int dx = k % 3 - 1, dy = k / 3 - 1;
			if ((dx | dy) != 0 && bit(wx + dx - px, wy + dy - py)) m |= 1u << k;
		}
		return m;
	}
};

__global__ __launch_bounds__(128)
void mvs_subpixel_search_kernel(const ViewDev *__restrict__ views, int ref, NeighList nl, int nneigh, srh_params P,
                                int y0, int nrows, int exhaustive, int32_t *__restrict__ win, int32_t *__restrict__ neigh,
                                uint8_t *__restrict__ cls, unsigned long long *__restrict__ cnt)
{
	const ViewDev &A = views[ref];
	const int W = A.w;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	unsigned fell = 0;
	if (q < (size_t)nrows*W) {
		const int x = (int)(q % W), y = y0 + (int)(q / W);
		const size_t pv = (size_t)y*W + x;
		int4 n = make_int4(-1, -1, -1, -1);
		int wi = -1, wx = -1, wy = -1;
		uint8_t k = SRH_SUBPX_NONE;
		const double z0 = A.depth[pv];
		if (A.mask[pv] == 1 && z0 > 0 && z0 < __builtin_inf()) {
			const double s = P.image_scale;
			const Ray ray = cam_unproject(A.cam, (x + 0.5) / s, (y + 0.5) / s);
			unsigned adj = 0;
			if (!exhaustive) {
				Vec3 X = load3(A.cam.C);
				if (point_from_depth(ray, load3(A.cam.pdir), z0, X)) {
					for (int i = 0; i < nneigh && wi < 0; ++i) {
						const ViewDev &B = views[nl.n[i]];
						Vec3 pr = X;
						if (!cam_project(B.cam, pr)) continue;
						const double x2 = pr.x*s, y2 = pr.y*s;
						if (!(fabs(x2) < 0x1p28 && fabs(y2) < 0x1p28)) continue;
						MvsNarrowVisitor vis = { A.cam, B.cam, P, ray, z0, (int)floor(x2), (int)floor(y2), -1, -1, false, 0ull, 0ull };
						walk_curve<true>(ray, A.cam, B, P, vis);
						if (vis.found) { wi = i; wx = vis.wx; wy = vis.wy; adj = vis.adjacency(); }
					}
				}
				if (wi < 0) fell = 1;
			}
			if (wi < 0) {
				for (int i = 0; i < nneigh && wi < 0; ++i) {
					const ViewDev &B = views[nl.n[i]];
					MvsWinnerVisitor vis = { A.cam, B.cam, P, ray, z0, -1, -1, false };
					walk_curve<true>(ray, A.cam, B, P, vis);
					if (vis.found) {
						wi = i; wx = vis.wx; wy = vis.wy;
						AdjacencyVisitor av = { wx, wy, 0u };
						walk_curve<true>(ray, A.cam, B, P, av);
						adj = av.mask;
					}
				}
			}
			k = SRH_SUBPX_NO_WINNER;
			if (wi >= 0) {
				const ViewDev &B = views[nl.n[wi]];
				double zm = -__builtin_inf(), zp = __builtin_inf();
				for (unsigned m = adj; m; m &= m - 1) {
					const int b = __builtin_ctz(m);
					const int qx = wx + b % 3 - 1, qy = wy + b / 3 - 1;
					const double z = candidate_depth(A.cam, B.cam, P, ray, qx, qy);
					if (z < z0 && z > zm) { zm = z; n.x = qx; n.y = qy; }
					if (z > z0 && z < zp) { zp = z; n.z = qx; n.w = qy; }
				}
				k = (n.x >= 0 && n.z >= 0) ? SRH_SUBPX_REFINED : SRH_SUBPX_NO_NEIGHBOUR;   // REFINED: provisional, the refine kernel decides
			}
		}
		win[3*pv] = wi; win[3*pv + 1] = wx; win[3*pv + 2] = wy;
		*reinterpret_cast<int4 *>(neigh + 4*pv) = n;
		cls[pv] = k;
	}
	block_count_add(cnt + 7, fell);
}

void launch_mvs_subpixel_search(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh_slots, int nneigh, int width,
                                const srh_params &P, int y0, int nrows, bool exhaustive, int32_t *win, int32_t *neigh,
                                uint8_t *cls, unsigned long long *cnt)
{
	if (nrows <= 0) return;
	const size_t n = (size_t)nrows*width;
	hipLaunchKernelGGL(mvs_subpixel_search_kernel, dim3((unsigned)((n + 127)/128)), dim3(128), 0, st,
	                   views, ref, make_neigh_list(neigh_slots, nneigh), nneigh, P, y0, nrows, exhaustive ? 1 : 0, win, neigh, cls, cnt);
}

__global__ __launch_bounds__(128)
void mvs_subpixel_refine_kernel(const ViewDev *__restrict__ views, int ref, NeighList nl, srh_params P, int y0, int nrows,
                                const double *__restrict__ wbuf, const int32_t *__restrict__ win,
                                const int32_t *__restrict__ neigh, uint8_t *__restrict__ cls, double *__restrict__ delta,
                                unsigned long long *__restrict__ cnt)
{
	__shared__ double cs[3][SRH_WTILE];
	__shared__ unsigned hist[SRH_MVSSUB_COUNTERS];
	const ViewDev &A = views[ref];
	const int W = A.w;
	const int tiles_per_row = (W + SRH_WTILE - 1)/SRH_WTILE;
	const int tid = threadIdx.x;
	const int role = tid >> 5, lx = tid & (SRH_WTILE - 1);          // 0: n-, 1: the winner, 2: n+, 3: idle
	const int trow = (int)(blockIdx.x / (unsigned)tiles_per_row);
	const int x = (int)(blockIdx.x % (unsigned)tiles_per_row)*SRH_WTILE + lx;
	const bool valid = trow < nrows && x < W;
	const int y = y0 + trow;
	const size_t pv = valid ? (size_t)y*W + x : 0;
	if (tid < SRH_MVSSUB_COUNTERS) hist[tid] = 0;
	uint8_t k = valid ? cls[pv] : (uint8_t)SRH_SUBPX_NONE;
	const bool pending = valid && k == SRH_SUBPX_REFINED;
	if (pending && role < 3) {
		const int wi = win[3*pv];
		const ViewDev &B = views[nl.n[wi]];
		const int2 c = role == 1 ? make_int2(win[3*pv + 1], win[3*pv + 2]) : *reinterpret_cast<const int2 *>(neigh + 4*pv + role);
		const int T = (2*P.window_radius + 1)*(2*P.window_radius + 1);
		cs[role][lx] = mvs_cost(A, B, wbuf + wbuf_offset(W, T, trow, x), SRH_WTILE, P, x, y, c.x, c.y);
	}
	__syncthreads();
	if (role == 0 && valid) {
		double d = 0.0;
		if (pending) {
			// classify(-c-, -c0, -c+) of srh_subpixel.hip: the cost here is higher-is-better
			const double cm = -cs[0][lx], c0 = -cs[1][lx], cp = -cs[2][lx];
			const double D = (cm - c0) + (cp - c0);
			k = SRH_SUBPX_FLAT;
			if (D > 0) {
				const double dl = 0.5*(cm - cp)/D;
				if (fabs(dl) <= 0.5) {
					k = SRH_SUBPX_REFINED;
					d = dl;
					if (dl != 0) {
						const ViewDev &B = views[nl.n[win[3*pv]]];
						const int wx = win[3*pv + 1], wy = win[3*pv + 2];
						const int2 n = *reinterpret_cast<const int2 *>(neigh + 4*pv + (dl > 0 ? 2 : 0));
						const double a = fabs(dl);
						const double qx = (wx + 0.5) + a*(double)(n.x - wx), qy = (wy + 0.5) + a*(double)(n.y - wy);
						const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
						A.depth[pv] = candidate_depth_at(A.cam, B.cam, P, ray, qx, qy);
						atomicAdd(&hist[6], 1u);
					}
				} else k = SRH_SUBPX_OUTSIDE;
			}
			cls[pv] = k;
		}
		delta[pv] = d;
		atomicAdd(&hist[k], 1u);
	}
	__syncthreads();
	if (tid < SRH_MVSSUB_COUNTERS - 1 && hist[tid]) atomicAdd(cnt + tid, (unsigned long long)hist[tid]);
}

void launch_mvs_subpixel_refine(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh_slots, int nneigh, int width,
                                const srh_params &P, int y0, int nrows, const double *wbuf, const int32_t *win,
                                const int32_t *neigh, uint8_t *cls, double *delta, unsigned long long *cnt)
{
	if (nrows <= 0) return;
	const unsigned tiles = (unsigned)((width + SRH_WTILE - 1)/SRH_WTILE);
	hipLaunchKernelGGL(mvs_subpixel_refine_kernel, dim3(tiles*(unsigned)nrows), dim3(128), 0, st,
	                   views, ref, make_neigh_list(neigh_slots, nneigh), P, y0, nrows, wbuf, win, neigh, cls, delta, cnt);
}

} // namespace srh
