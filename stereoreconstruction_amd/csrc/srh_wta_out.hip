// srh_wta_out.hip -- the exact costs of the winner-take-all scan's by-products (option "wta_outputs").
//
// The scan kernels keep WHICH candidate won and which one held the minimum before it (wta_store, srh_internal.hpp); the
// costs they compared are, under the certified arithmetic, fused approximations whose decisions are proven and whose
// numbers are not the reference's.  So the two costs of a pixel are evaluated here, once, in the reference's arithmetic:
// tv_cost / tv_cost_sad / tv_cost_census of srh_walk.hpp, the functions pair_costs_kernel evaluates -- the same operations in the same
// order under -ffp-contract=off, hence the same bits, whatever arithmetic chose the winner.
//
// Launched per band on the pass's stream behind the last kernel that can still change the band's winners (the scan, its
// flagged redo, its rescan), while the band's window buffer is still intact: no window is rebuilt.  One wave per window
// tile (32 consecutive pixels of a row): lanes 0-31 take the tile's winners, lanes 32-63 its runners-up, so a tap of the
// window is one 256-byte line (tile-major layout) shared by both half-waves; the other view's taps are gathers at two
// unrelated places per pixel.  A pixel or a slot without a candidate stores +INF and evaluates nothing.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"

namespace srh {

__global__ __launch_bounds__(64)
void twoview_winner_costs_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P, int kind,
                                 int y0, int nrows, const double *__restrict__ wbuf, int wimg,
                                 const int32_t *__restrict__ wout, double *__restrict__ min_cost, double *__restrict__ second_cost)
{
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w;
	const int tiles_per_row = (W + SRH_WTILE - 1)/SRH_WTILE;
	const int lane = threadIdx.x;
	const int trow = (int)(blockIdx.x / (unsigned)tiles_per_row);
	const int x = (int)(blockIdx.x % (unsigned)tiles_per_row)*SRH_WTILE + (lane & (SRH_WTILE - 1));
	const int which = lane >> 5;                                      // 0: the winner, 1: the runner-up
	if (trow >= nrows || x >= W) return;
	const int y = y0 + trow;
	const size_t npix = (size_t)W*L.h, pv = (size_t)y*W + x;
	const int2 c = *reinterpret_cast<const int2 *>(wout + 2*((size_t)which*npix + pv));
	double v = __builtin_inf();
	if (c.x >= 0 && c.y >= 0) {
		const int R = P.window_radius, WS = 2*R + 1;
		if (wimg) {
			const double *wq = wbuf + wimg_offset(W, R, trow, x);
			v = tv_cost_of(kind, L, Rv, wq, 1, P, x, y, c.x, c.y, (size_t)wimg_row_stride(R));
		} else {
			const double *wq = wbuf + wbuf_offset(W, WS*WS, trow, x);
			v = tv_cost_of(kind, L, Rv, wq, SRH_WTILE, P, x, y, c.x, c.y);
		}
	}
	(which ? second_cost : min_cost)[pv] = v;
}

void launch_twoview_winner_costs(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int kind,
                                 int y0, int nrows, const double *wbuf, bool wimg, const int32_t *wout,
                                 double *min_cost, double *second_cost)
{
	if (nrows <= 0) return;
	const unsigned tiles = (unsigned)((width + SRH_WTILE - 1)/SRH_WTILE);
	hipLaunchKernelGGL(twoview_winner_costs_kernel, dim3(tiles*(unsigned)nrows), dim3(64), 0, st,
	                   views, ref, oth, P, kind, y0, nrows, wbuf, wimg ? 1 : 0, wout, min_cost, second_cost);
}

} // namespace srh
