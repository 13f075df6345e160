// srh_subpixel.hip -- sub-pixel depth from the winner's neighbours on the curve (option "subpixel").
//
// The winner-take-all scan stores candidate_depth of an integer pixel of the other view: one disparity step.  With the
// option a pass refines each pixel it has decided, band by band, behind twoview_winner_costs_kernel -- that is, behind the
// last kernel that can change the band's winners or depths, while the band's window buffer is intact:
//
//   1. S = the pixels walk_curve<false> visits for the reference pixel (order and multiplicity ignored), A = the members of
//      S at Chebyshev distance 1 from the kept winner w.  Of A, scanned in ascending (qy, qx), n- is the q with the largest
//      candidate_depth(q) < z0 and n+ the one with the smallest candidate_depth(q) > z0 (strict comparisons: the first q met
//      wins a tie; a q at z0 or with a NaN depth is on neither side).  z0 is the pixel's depth as the scan left it.
//   2. cm, c0, cp = the reference-form cost (tv_cost_of under the pass's cost kind: the bits of pair_costs_kernel) of the pixel against
//      n-, w, n+; c0 is the kept min_cost.
//   3. D = (cm - c0) + (cp - c0); delta = 0.5*(cm - cp)/D; refined when D > 0 and |delta| <= 0.5.  The new depth is
//      candidate_depth at w + |delta|*(n - w), n = n+ for delta > 0, else n-; delta == 0 keeps the depth's bits.
//
// Two kernels.  subpixel_neighbours_kernel (one lane per pixel) walks the curve with a visitor that keeps an 8-bit adjacency
// mask around the winner -- no list, no sort -- and evaluates at most eight candidate depths.  subpixel_refine_kernel is
// shaped like twoview_winner_costs_kernel: one wave per 32-pixel window tile, lanes 0-31 take n-, lanes 32-63 n+, the two
// half-waves swap their costs across lanes, and the lower half finishes delta, the class and the depth.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_depth_at.hpp"
#include "srh_subpixel.hpp"

namespace srh {

// (candidate_depth_at and AdjacencyVisitor: srh_depth_at.hpp, shared with srh_mvs_subpixel.hip)

__global__ __launch_bounds__(128)
void subpixel_neighbours_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P, int y0, int nrows,
                                const double *__restrict__ tdist, const int32_t *__restrict__ win_xy,
                                int32_t *__restrict__ neigh, uint8_t *__restrict__ cls)
{
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (q >= (size_t)nrows*W) return;
	const int x = (int)(q % W), y = y0 + (int)(q / W);
	const size_t pv = (size_t)y*W + x;
	int4 n = make_int4(-1, -1, -1, -1);
	uint8_t k = SRH_SUBPX_NONE;
	const int2 w = *reinterpret_cast<const int2 *>(win_xy + 2*pv);
	const double z0 = L.depth[pv];
	if (L.mask[pv] == 1 && w.x >= 0 && w.y >= 0 && fabs(z0) < __builtin_inf()) {
		const Ray ray = cam_unproject(L.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
		AdjacencyVisitor vis = { w.x, w.y, 0u };
		walk_curve<false>(ray, L.cam, Rv, P, vis, tdist);
		double zm = -__builtin_inf(), zp = __builtin_inf();
		for (unsigned m = vis.mask; m; m &= m - 1) {
			const int b = __builtin_ctz(m);
			const int qx = w.x + b % 3 - 1, qy = w.y + b / 3 - 1;
			const double z = candidate_depth(L.cam, Rv.cam, P, ray, qx, qy);
			if (z < z0 && z > zm) { zm = z; n.x = qx; n.y = qy; }
			if (z > z0 && z < zp) { zp = z; n.z = qx; n.w = qy; }
		}
		k = (n.x >= 0 && n.z >= 0) ? SRH_SUBPX_REFINED : SRH_SUBPX_NO_NEIGHBOUR;   // REFINED: provisional, the refine kernel decides
	}
	*reinterpret_cast<int4 *>(neigh + 4*pv) = n;
	cls[pv] = k;
}

void launch_subpixel_neighbours(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                int y0, int nrows, const double *tdist, const int32_t *win_xy, int32_t *neigh, uint8_t *cls)
{
	if (nrows <= 0) return;
	const size_t n = (size_t)nrows*width;
	hipLaunchKernelGGL(subpixel_neighbours_kernel, dim3((unsigned)((n + 127)/128)), dim3(128), 0, st,
	                   views, ref, oth, P, y0, nrows, tdist, win_xy, neigh, cls);
}

__global__ __launch_bounds__(64)
void subpixel_refine_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P, int kind,
                            int y0, int nrows, const double *__restrict__ wbuf, int wimg,
                            const int32_t *__restrict__ win_xy, const double *__restrict__ min_cost,
                            const int32_t *__restrict__ neigh, uint8_t *__restrict__ cls, double *__restrict__ delta)
{
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w;
	const int tiles_per_row = (W + SRH_WTILE - 1)/SRH_WTILE;
	const int lane = threadIdx.x;
	const int trow = (int)(blockIdx.x / (unsigned)tiles_per_row);
	const int x = (int)(blockIdx.x % (unsigned)tiles_per_row)*SRH_WTILE + (lane & (SRH_WTILE - 1));
	const int which = lane >> 5;                                      // 0: n-, 1: n+
	if (trow >= nrows || x >= W) return;                              // (both lanes of a pixel leave together)
	const int y = y0 + trow;
	const size_t pv = (size_t)y*W + x;
	const bool pending = cls[pv] == SRH_SUBPX_REFINED;
	double v = 0.0;
	if (pending) {
		const int2 c = *reinterpret_cast<const int2 *>(neigh + 4*pv + 2*which);
		const int R = P.window_radius, WS = 2*R + 1;
		if (wimg) {
			const double *wq = wbuf + wimg_offset(W, R, trow, x);
			v = tv_cost_of(kind, L, Rv, wq, 1, P, x, y, c.x, c.y, (size_t)wimg_row_stride(R));
		} else {
			const double *wq = wbuf + wbuf_offset(W, WS*WS, trow, x);
			v = tv_cost_of(kind, L, Rv, wq, SRH_WTILE, P, x, y, c.x, c.y);
		}
	}
	// the other half-wave's cost of the same pixel: lane ^ 32 (both are here, see above)
	const double u = __shfl_xor(v, 32);
	if (which) return;
	double d = 0.0;
	if (pending) {
		const double cm = v, cp = u, c0 = min_cost[pv];
		const double D = (cm - c0) + (cp - c0);
		uint8_t k = SRH_SUBPX_FLAT;
		if (D > 0) {
			const double dl = 0.5*(cm - cp)/D;
			if (fabs(dl) <= 0.5) {
				k = SRH_SUBPX_REFINED;
				d = dl;
				if (dl != 0) {
					const int2 w = *reinterpret_cast<const int2 *>(win_xy + 2*pv);
					const int2 n = *reinterpret_cast<const int2 *>(neigh + 4*pv + (dl > 0 ? 2 : 0));
					const double a = fabs(dl);
					const double qx = (w.x + 0.5) + a*(double)(n.x - w.x), qy = (w.y + 0.5) + a*(double)(n.y - w.y);
					const Ray ray = cam_unproject(L.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
					L.depth[pv] = candidate_depth_at(L.cam, Rv.cam, P, ray, qx, qy);
				}
			} else k = SRH_SUBPX_OUTSIDE;
		}
		cls[pv] = k;
	}
	delta[pv] = d;
}

void launch_subpixel_refine(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int kind,
                            int y0, int nrows, const double *wbuf, bool wimg, const int32_t *win_xy, const double *min_cost,
                            const int32_t *neigh, uint8_t *cls, double *delta)
{
	if (nrows <= 0) return;
	const unsigned tiles = (unsigned)((width + SRH_WTILE - 1)/SRH_WTILE);
	hipLaunchKernelGGL(subpixel_refine_kernel, dim3(tiles*(unsigned)nrows), dim3(64), 0, st,
	                   views, ref, oth, P, kind, y0, nrows, wbuf, wimg ? 1 : 0, win_xy, min_cost, neigh, cls, delta);
}

} // namespace srh
