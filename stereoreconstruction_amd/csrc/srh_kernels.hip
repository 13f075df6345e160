// srh_kernels.hip -- gfx950 kernels of the dense matching-cost / support-weight /
// winner-take-all path.  IEEE double in the reference's operation order; built
// with -ffp-contract=off.
//
// General ("curve walk") kernels, one thread per reference pixel:
//   prep_view_kernel            gray / TwoView-tap-validity planes         
//   weights_kernel              Geodesic / Adaptive support windows        (#2, #3)
//   twoview_generic_kernel      epipolarCurve + cost_ncc + running-min WTA (#6-#10)
//   twoview_cross_check_kernel                                             (#11)
// and the point cloud, epipolar preview / curves and refraction error kernels of the GUI's requests.
// The dense row-aligned TwoView kernels live in srh_dense.hip, MultiViewStereo's in srh_mvs.hip.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_window.hpp"

#include <cstdlib>

namespace srh {

static inline int grid_for(size_t n, int block, int cap) {
	size_t b = (n + block - 1)/block;
	if (b > (size_t)cap) b = cap;
	if (b < 1) b = 1;
	return (int)b;
}

// ------------------------------------------------------------------ prep
// util/vectorimage.hpp:60-62 toGray; vectorimage.cpp:129-155 sample() validity at
// integer coordinates (x+1 < w && y+1 < h), where sample() returns pixel() exactly.
__global__ void prep_view_kernel(const uint32_t *__restrict__ rgba, const uint8_t *__restrict__ mask,
                                 int w, int h, double *__restrict__ gray, double *__restrict__ gray_tv)
{
	const size_t n = (size_t)w*h;
	for (size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x*blockDim.x) {
		const uint32_t px = rgba[i];
		const double r = (double)(px & 255u), g = (double)((px >> 8) & 255u), b = (double)((px >> 16) & 255u);
		const double gr = (0.11*r + 0.59*g + 0.3*b);
		const int x = (int)(i % (size_t)w), y = (int)(i / (size_t)w);
		gray[i] = gr;
		const bool ok = mask[i] == 1 && x + 1 < w && y + 1 < h;
		gray_tv[i] = ok ? gr : __builtin_nan("");
	}
}

__global__ void fill_kernel(double *__restrict__ p, size_t n, double v) {
	for (size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x*blockDim.x)
		p[i] = v;
}

void launch_prep_view(hipStream_t st, const uint32_t *rgba, const uint8_t *mask, int w, int h,
                      double *gray, double *gray_tv)
{
	hipLaunchKernelGGL(prep_view_kernel, dim3(grid_for((size_t)w*h, 256, 2048)), dim3(256), 0, st,
	                   rgba, mask, w, h, gray, gray_tv);
}

void launch_fill(hipStream_t st, double *p, size_t n, double v) {
	hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, st, p, n, v);
}

// ------------------------------------------------------------------ weights
// (the window itself: support_window, srh_window.hpp)
// Any-radius version: the window lives in the global weight buffer
// (tile-major layout of srh_internal.hpp: wb[tap*wstride], wstride = SRH_WTILE; or, wimg != 0, the
// strip kernel's LDS-image layout: wb[row*32*WP + col]).
__global__ void weights_kernel(const ViewDev *__restrict__ views, int ref, srh_params P,
                               int y0, int nrows, double *__restrict__ wbuf, size_t wstride, double *__restrict__ pconst,
                               int wimg)
{
	const ViewDev &V = views[ref];
	const int W = V.w, H = V.h;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (q >= (size_t)nrows*W) return;
	const int cx = (int)(q % W), cy = y0 + (int)(q / W);
	if (V.mask[(size_t)cy*W + cx] != 1) return;                 // masked pixels never reach init_weights
	const int R = P.window_radius, WS = 2*R + 1;
	double *wb = wbuf + (wimg ? wimg_offset(W, R, (int)(q / W), cx) : wbuf_offset(W, WS*WS, (int)(q / W), cx));
	// tap (r, c) of the window at wb[r*wrs + c*wcs]
	const size_t wrs = wimg ? (size_t)wimg_row_stride(R) : (size_t)WS*wstride, wcs = wimg ? 1 : wstride;
#define WTAP(r, c) wb[(size_t)(r)*wrs + (size_t)(c)*wcs]

	support_window(V, P, cx, cy, [&](int r, int c) -> double & { return WTAP(r, c); });
	if (pconst) {
		// per-pixel constants of the dense kernel's fast cost form (see geodesic_reg_kernel): same taps, same order
		bool all = true;
		double mL = 0, tw = 0;
		for (int row = -R; row <= R; ++row)
			for (int col = -R; col <= R; ++col) {
				const int px = cx + col, py = cy + row;
				const double gl = (px < 0 || py < 0 || px >= W || py >= H) ? __builtin_nan("") : V.gray_tv[(size_t)py*W + px];
				const double wt = WTAP(row + R, col + R);
				if (!(gl == gl && wt > P.weight_cutoff)) all = false;
				mL += wt*gl;
				tw += wt;
			}
		double s2 = 0, sa = 0;
		if (all && !(tw < 1e-10)) {
			mL /= tw;
			for (int row = -R; row <= R; ++row)
				for (int col = -R; col <= R; ++col) {
					const double wt_ = WTAP(row + R, col + R), gl_ = V.gray_tv[(size_t)(cy + row)*W + (cx + col)];
					const double t = wt_*gl_ - mL;
					s2 += t*t;
					sa += __builtin_fma(wt_, gl_, -mL);                      // (fused: srh_internal.hpp, SRH_PC)
				}
		} else all = false;
		pconst_store(pconst + ((size_t)(q / W)*W + cx)*SRH_PC, PixelConstants{ mL, tw, s2, sa, all });
	}
#undef WTAP
}

void launch_weights(hipStream_t st, const ViewDev *views, int ref, int width, const srh_params &P,
                    int y0, int nrows, double *wbuf, size_t wstride, double *pconst, bool wimg)
{
	const size_t n = (size_t)nrows*width;
	hipLaunchKernelGGL(weights_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st,
	                   views, ref, P, y0, nrows, wbuf, wstride, pconst, wimg ? 1 : 0);
}

// ------------------------------------------------------------------ TwoView, general geometry
// the rule and its state: srh_wta.hpp (WTA, option "wta_outputs": the runner-up travels along)
template <int KIND, bool WTA>
struct TwoViewDirectVisitor {
	const ViewDev &L, &Rv;
	const double *wq;
	size_t wstride;
	const srh_params &P;
	int x, y;
	WtaState<WtaXY, WTA> st;
	unsigned n;
	__device__ __forceinline__ void operator()(int cx, int cy) {
		const double cost = tv_cost_of(KIND, L, Rv, wq, wstride, P, x, y, cx, cy);
		++n;
		st.take(cost, WtaXY{ cx, cy }, P.wta_margin);
	}
};

// KIND: the cost (option "cost", SRH_COST_*); WTA: winner and runner-up into wout (wta_store)
template <int KIND, bool WTA>
__global__ void twoview_generic_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P,
                                       int y0, int nrows, const double *__restrict__ wbuf, size_t wstride,
                                       Counters *__restrict__ cnt, int32_t *__restrict__ wout)
{
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	unsigned n_eval = 0, n_pix = 0;
	if (q < (size_t)nrows*W) {
		const int x = (int)(q % W), y = y0 + (int)(q / W);
		const size_t pv = (size_t)y*W + x;
		double depth = __builtin_nan("");                       // twoviewstereo.cpp:269
		int ox = -1, oy = -1, rx = -1, ry = -1;
		if (L.mask[pv] == 1) {
			n_pix = 1;
			const Ray ray = cam_unproject(L.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
			const int T = (2*P.window_radius + 1)*(2*P.window_radius + 1);
			TwoViewDirectVisitor<KIND, WTA> vis = { L, Rv, wbuf + wbuf_offset(W, T, (int)(q / W), x), wstride, P, x, y,
			                             WtaState<WtaXY, WTA>(WtaXY{ -1, -1 }), 0 };
			walk_curve<false>(ray, L.cam, Rv, P, vis);
			n_eval = vis.n;
			if (WTA) { ox = vis.st.win.x; oy = vis.st.win.y; rx = vis.st.run.x; ry = vis.st.run.y; }
			if (vis.st.win.x >= 0)                                 // at least one candidate was scanned
				depth = candidate_depth(L.cam, Rv.cam, P, ray, vis.st.win.x, vis.st.win.y);
			if (vis.st.rejected(P.second_best_factor))
				depth = __builtin_inf();
		}
		L.depth[pv] = depth;
		if (WTA) wta_store(wout, (size_t)W*L.h, pv, ox, oy, rx, ry);
	}
	block_count_add(&cnt->n_eval, n_eval);
	block_count_add(&cnt->n_eval_device, n_eval);
	block_count_add(&cnt->n_pixels, n_pix);
}

void launch_twoview_generic(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                            int y0, int nrows, const double *wbuf, size_t wstride, Counters *cnt, int kind, int32_t *wout)
{
	const size_t n = (size_t)nrows*width;
	const dim3 grid((unsigned)((n + 127)/128)), block(128);
#define SRH_GEN_LAUNCH(S_, W_) hipLaunchKernelGGL((twoview_generic_kernel<S_, W_>), grid, block, 0, st, views, ref, oth, P, y0, nrows, wbuf, wstride, cnt, wout)
	if (kind == SRH_COST_SAD)         { if (wout) SRH_GEN_LAUNCH(SRH_COST_SAD, true); else SRH_GEN_LAUNCH(SRH_COST_SAD, false); }
	else if (kind == SRH_COST_CENSUS) { if (wout) SRH_GEN_LAUNCH(SRH_COST_CENSUS, true); else SRH_GEN_LAUNCH(SRH_COST_CENSUS, false); }
	else                              { if (wout) SRH_GEN_LAUNCH(SRH_COST_NCC, true); else SRH_GEN_LAUNCH(SRH_COST_NCC, false); }
#undef SRH_GEN_LAUNCH
}

// one direction of TwoViewStereo::crossCheck (twoviewstereo.cpp:604-636 / :638-670)
__global__ void twoview_cross_check_kernel(const ViewDev *__restrict__ views, int self, int other, srh_params P)
{
	const ViewDev &A = views[self];
	const ViewDev &B = views[other];
	const int W = A.w, H = A.h;
	const size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= (size_t)W*H) return;
	const int x = (int)(i % W), y = (int)(i / W);
	double depth = A.depth[i];
	if (!isfinite_d(depth)) return;
	const double s = P.image_scale;
	const double inf = __builtin_inf();
	const Ray ray = cam_unproject(A.cam, (x + 0.5) / s, (y + 0.5) / s);
	Vec3 p1 = load3(A.cam.C);
	if (point_from_depth(ray, load3(A.cam.pdir), depth, p1)) {
		Vec3 q = p1;
		if (cam_project(B.cam, q)) {
			const double x2 = q.x*s, y2 = q.y*s;
			// CONTAINS(resultRight, x2, y2) and PV(x2, y2, resultRight), twoviewstereo.cpp:621-622
			if (x2 >= 0 && y2 >= 0 && x2 < B.w && y2 < B.h) {
				const double odepth = B.depth[(size_t)((int)y2)*B.w + (int)x2];
				if (isfinite_d(odepth)) {
					const Ray ray2 = cam_unproject(B.cam, (x2 + 0.5) / s, (y2 + 0.5) / s);
					Vec3 p2 = load3(B.cam.C);
					if (point_from_depth(ray2, load3(B.cam.pdir), odepth, p2)) {
						const double nrm = norm(p1 - p2);
						if (!isfinite_d(nrm) || nrm > P.inconsistency_thresh) depth = inf;
					} else depth = inf;
				} else depth = inf;
			} else depth = inf;
		} else depth = inf;
	}
	A.depth[i] = depth;
}

void launch_twoview_cross_check(hipStream_t st, const ViewDev *views, int self, int other, int w, int h,
                                const srh_params &P)
{
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(twoview_cross_check_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st,
	                   views, self, other, P);
}

// ------------------------------------------------------------------ depth map -> point cloud
// one thread per pixel: unproject + pointFromDepth (the cross-checks' construction, twoviewstereo.cpp:612-614)
__global__ void point_cloud_kernel(const ViewDev *__restrict__ views, int slot, srh_params P,
                                   double *__restrict__ xyz, uint8_t *__restrict__ rgb, uint8_t *__restrict__ valid,
                                   unsigned long long *__restrict__ counts)
{
	const ViewDev &A = views[slot];
	const int W = A.w, H = A.h;
	const size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	unsigned n_pt = 0, n_mask = 0, n_fin = 0;
	if (i < (size_t)W*H) {
		const int x = (int)(i % W), y = (int)(i / W);
		const double nanv = __builtin_nan("");
		Vec3 pt = v3(nanv, nanv, nanv);
		bool ok = false;
		if (A.mask[i] == 1) {
			n_mask = 1;
			const double depth = A.depth[i];
			if (isfinite_d(depth)) {
				n_fin = 1;
				const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
				Vec3 q = load3(A.cam.C);
				if (point_from_depth(ray, load3(A.cam.pdir), depth, q)) { pt = q; ok = true; n_pt = 1; }
			}
		}
		if (xyz) { xyz[3*i] = pt.x; xyz[3*i + 1] = pt.y; xyz[3*i + 2] = pt.z; }
		if (rgb) { const uint32_t c = A.rgba[i]; rgb[3*i] = (uint8_t)(c & 255u); rgb[3*i + 1] = (uint8_t)((c >> 8) & 255u); rgb[3*i + 2] = (uint8_t)((c >> 16) & 255u); }
		if (valid) valid[i] = ok ? 1 : 0;
	}
	block_count_add(&counts[0], n_pt);
	block_count_add(&counts[1], n_mask);
	block_count_add(&counts[2], n_fin);
}

void launch_point_cloud(hipStream_t st, const ViewDev *views, int slot, int w, int h, const srh_params &P,
                        double *xyz, uint8_t *rgb, uint8_t *valid, unsigned long long *counts)
{
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(point_cloud_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st, views, slot, P, xyz, rgb, valid, counts);
}

// ------------------------------------------------------------------ GUI-side users of the camera model
// StereoWidget::epipolarLineItem (gui/widgets/stereowidget.cpp:621-672): one thread per queried pixel
__global__ void epipolar_preview_kernel(const ViewDev *__restrict__ views, int ref, int oth, double min_depth, double max_depth,
                                        int num_depths, int nq, const double *__restrict__ xy, double *__restrict__ out,
                                        int32_t *__restrict__ counts)
{
	const int q = blockIdx.x*blockDim.x + threadIdx.x;
	if (q >= nq) return;
	const srh_camera &L = views[ref].cam, &Rc = views[oth].cam;
	const Ray ray = cam_unproject(L, xy[2*q], xy[2*q + 1]);           // the pixel as given: no +0.5, no scale
	const Vec3 n = normalized(load3(L.pdir));                           // Plane3d(direction, depth)
	double *o = out + (size_t)q*2*num_depths;
	int nv = 0;
	bool first = true;
	double p1x = __builtin_nan(""), p1y = 0;
	for (int k = 0; k < num_depths; ++k) {
		const double t = k / (num_depths - 1.0);
		const double depth = min_depth*(1 - t) + max_depth*t;
		Vec3 p2;
		if (!intersect_plane(ray, n, depth, p2)) continue;
		if (!cam_project(Rc, p2)) continue;
		if (isnan_d(p1x)) { p1x = p2.x; p1y = p2.y; }
		const double dx = p2.x - p1x, dy = p2.y - p1y;
		if ((dx*dx + dy*dy) > 1) {
			if (first) { o[2*nv] = p1x; o[2*nv + 1] = p1y; ++nv; first = false; }
			o[2*nv] = p2.x; o[2*nv + 1] = p2.y; ++nv;
			p1x = p2.x; p1y = p2.y;
		}
	}
	counts[q] = nv;
}

// RefractiveCalibrationFunction::diff (stereo/refractioncalibration.cpp:175-199): one thread per correspondence
__global__ void refraction_error_kernel(const ViewDev *__restrict__ views, int v1, int v2, int n,
                                        const double *__restrict__ p1, const double *__restrict__ p2, double *__restrict__ err)
{
	const int i = blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	const srh_camera &A = views[v1].cam, &B = views[v2].cam;
	const Ray R1 = cam_unproject(A, p1[2*i], p1[2*i + 1]);
	const Ray R2 = cam_unproject(B, p2[2*i], p2[2*i + 1]);
	Vec3 q1, q2;
	closest_points(R1, R2, q1, q2);
	const double out = norm(q1 - q2);
	const Vec3 mid = (q1 + q2)*0.5;
	const double e1 = (0.5 * A.K[0] * out) / cam_local_z(A, mid);
	const double e2 = (0.5 * B.K[0] * out) / cam_local_z(B, mid);
	err[i] = e1 + e2;
}

void launch_epipolar_preview(hipStream_t st, const ViewDev *views, int ref, int oth, double zmin, double zmax, int nd,
                             int nq, const double *xy, double *out, int32_t *counts)
{
	hipLaunchKernelGGL(epipolar_preview_kernel, dim3((unsigned)((nq + 63)/64)), dim3(64), 0, st, views, ref, oth, zmin, zmax, nd, nq, xy, out, counts);
}

void launch_refraction_error(hipStream_t st, const ViewDev *views, int v1, int v2, int n, const double *p1, const double *p2, double *err)
{
	hipLaunchKernelGGL(refraction_error_kernel, dim3((unsigned)((n + 127)/128)), dim3(128), 0, st, views, v1, v2, n, p1, p2, err);
}

// ------------------------------------------------------------------ epipolar curves on request
struct CurveWriter {
	int32_t *out;
	int cap, n;
	__device__ __forceinline__ void operator()(int cx, int cy) {
		if (n < cap) { out[2*n] = cx; out[2*n + 1] = cy; }
		++n;
	}
};

// one thread per queried pixel (the GUI asks for one curve at a time; tests for a few hundred)
__global__ void epipolar_curves_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P, int mvs,
                                       int nq, const int32_t *__restrict__ xy, int32_t *__restrict__ out, int cap,
                                       int32_t *__restrict__ counts)
{
	const int q = blockIdx.x*blockDim.x + threadIdx.x;
	if (q >= nq) return;
	const ViewDev &L = views[ref];
	const Ray ray = cam_unproject(L.cam, (xy[2*q] + 0.5) / P.image_scale, (xy[2*q + 1] + 0.5) / P.image_scale);
	CurveWriter wr = { out + (size_t)q*2*cap, cap, 0 };
	if (mvs) walk_curve<true>(ray, L.cam, views[oth], P, wr);
	else walk_curve<false>(ray, L.cam, views[oth], P, wr);
	counts[q] = wr.n;
}

void launch_epipolar_curves(hipStream_t st, const ViewDev *views, int ref, int oth, const srh_params &P, int mvs,
                            int nq, const int32_t *xy, int32_t *out, int cap, int32_t *counts)
{
	hipLaunchKernelGGL(epipolar_curves_kernel, dim3((unsigned)((nq + 63)/64)), dim3(64), 0, st,
	                   views, ref, oth, P, mvs, nq, xy, out, cap, counts);
}

} // namespace srh
