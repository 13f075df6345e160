// srh_rectify.hpp -- rectification of a verged, distorted pair onto the dense row-aligned plan: the rig test
// that proposes the dense plan, the rectifying geometry, and the per-pixel pieces of the warp (srh_twoview_rectify,
// srh_view_rectify_map) and of the way back (srh_view_depth_unrectify).  Usable from host and gfx950 device code:
// srh_rectify.hip runs the per-pixel pieces one lane per pixel, srh_api.hip the geometry, and the CPU suite compiles this
// header with g++ and holds both against numpy (tests/rectify_host.cpp, tests/test_rectify_host.py).
// IEEE double throughout, no fused multiply-add (the translation units are built with -ffp-contract=off).
#pragma once

#include "srh_geom.hpp"

namespace srh {

// Can every epipolar curve of `a` in `b` stay on its own image row?  Undistorted, non-refractive
// cameras with the same orientation and the same second and third rows of K, displaced along the
// camera x axis.  K's FIRST row is not compared: fx and cx may differ per view (srh_twoview_rectify hands over one cx per
// view), and then a pixel's candidates are no fixed shift of x -- with fx_b != fx_a they slide by (fx_b/fx_a - 1)(x - cx_a).
// fx_bx = |fx_b * baseline| is the widest range in columns per unit of inverse depth, the plan's stride.
// This only *proposes* the dense path.  What keeps a proposal right, or refutes it: every pixel's column range is its own
// (pinhole_column_range projects the pixel's own ray at both ends of the depth range with the other view's K), the scan
// counts a candidate off its row or outside that range (`ty != y || tx < lo || tx > hi`, Counters::not_row_aligned) and the
// driver then repeats the pass on the general kernels, and the template scan serves a pixel only under its per-pixel bound
// or its label-by-label tier (ts_pixel_passes), which know nothing of the rig.  tests/test_gpu_rigs.py holds all of it to
// the oracle on the rigs of tests/rig_cases.py.
// (srh_twoview_row_aligned exports it; TvPass::plan calls it.)
inline bool rig_is_row_aligned(const srh_camera &a, const srh_camera &b, double *fx_bx) {
	if (a.is_distorted || b.is_distorted || a.is_refractive || b.is_refractive) return false;
	for (int k = 0; k < 9; ++k) if (fabs(a.R[k] - b.R[k]) > 1e-13) return false;
	for (int k = 3; k < 9; ++k) if (fabs(a.K[k] - b.K[k]) > 1e-9*(1.0 + fabs(a.K[k]))) return false;
	if (fabs(a.K[1]) > 1e-12 || fabs(b.K[1]) > 1e-12 || fabs(a.K[3]) > 1e-12 || fabs(a.K[6]) > 1e-12 || fabs(a.K[7]) > 1e-12)
		return false;
	const Vec3 d = load3(b.C) - load3(a.C);
	const Vec3 bc = matvec(a.R, d);                               // baseline in camera axes
	const double len = norm(bc);
	if (!(len > 0) || fabs(bc.y) > 1e-12*len || fabs(bc.z) > 1e-12*len) return false;
	*fx_bx = fabs(b.K[0]*bc.x);
	return true;
}

namespace rect {

SRH_HD Vec3 cross(Vec3 a, Vec3 b) { return v3(a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x); }

// What srh_camera_from_krt is handed for the two rectified cameras: one rotation, one K per view, t_v = -Rn*C_v
struct Geometry { double Rn[9], Ka[9], Kb[9], ta[3], tb[3]; };

// The rectifying geometry of the pair (a, b), whose (scaled) images are w x h, for the parameters r.  SRH_OK, or the
// refusal's code with its reason in *why.
//   r1 = (C_b - C_a)/|C_b - C_a|, negated where it points against the cameras' x axes
//   k  = sum of the two optical axes;  r2 = cross(k, r1) normalised;  r3 = cross(r1, r2);  Rn = rows r1, r2, r3
//   Kn_v = [[f, 0, cx_v], [0, f, cy], [0, 0, 1]]:  auto f = mean of the four focal lengths;  with d_v = Rn * (optical axis
//   of v):  auto cx_v = (out_w/scale)/2 - f*d_v.x/d_v.z (the old optical axis lands on the middle column),  auto
//   cy = (out_h/scale)/2 - f*mean_v(d_v.y/d_v.z);  SRH_RECTIFY_SHARED_CX: both auto cx_v replaced by their mean
inline int geometry(const srh_camera &a, const srh_camera &b, int w, int h, double image_scale, const srh_rectify_params &r,
                    Geometry &g, const char **why)
{
	*why = "";
	if (w <= 0 || h <= 0) { *why = "bad view size"; return SRH_E_INVALID; }
	if (!(image_scale > 0) || !isfinite_d(image_scale)) { *why = "image_scale must be > 0"; return SRH_E_INVALID; }
	if (r.out_w < 0 || r.out_h < 0 || r.out_w > SRH_MAX_VIEW_DIM || r.out_h > SRH_MAX_VIEW_DIM) { *why = "bad output size"; return SRH_E_INVALID; }
	if (r.flags & ~SRH_RECTIFY_SHARED_CX) { *why = "unknown flag bits"; return SRH_E_INVALID; }
	if (!(r.focal >= 0) || !isfinite_d(r.focal)) { *why = "focal must be finite and >= 0"; return SRH_E_INVALID; }
	if ((!isnan_d(r.cx_a) && !isfinite_d(r.cx_a)) || (!isnan_d(r.cx_b) && !isfinite_d(r.cx_b)) || (!isnan_d(r.cy) && !isfinite_d(r.cy))) {
		*why = "principal point must be finite (or NaN: auto)"; return SRH_E_INVALID;
	}
	if (a.is_refractive || b.is_refractive) { *why = "a refractive camera has no rectifying homography"; return SRH_E_UNSUPPORTED; }
	const Vec3 Ca = load3(a.C), Cb = load3(b.C);
	const Vec3 base = Cb - Ca;
	const double len = norm(base);
	if (!(len > 0) || !isfinite_d(len)) { *why = "coincident camera centres"; return SRH_E_INVALID; }
	Vec3 r1 = v3(base.x/len, base.y/len, base.z/len);
	if (dot(r1, load3(a.R) + load3(b.R)) < 0) r1 = v3(-r1.x, -r1.y, -r1.z);
	const Vec3 k = load3(a.R + 6) + load3(b.R + 6);
	const Vec3 kr = cross(k, r1);
	const double kn = norm(k), krn = norm(kr);
	if (!(kn > 0) || !(krn >= 1e-6*kn)) { *why = "the baseline runs along the viewing direction (forward motion)"; return SRH_E_UNSUPPORTED; }
	const Vec3 r2 = v3(kr.x/krn, kr.y/krn, kr.z/krn);
	const Vec3 r3 = cross(r1, r2);
	g.Rn[0] = r1.x; g.Rn[1] = r1.y; g.Rn[2] = r1.z;
	g.Rn[3] = r2.x; g.Rn[4] = r2.y; g.Rn[5] = r2.z;
	g.Rn[6] = r3.x; g.Rn[7] = r3.y; g.Rn[8] = r3.z;
	const Vec3 da = matvec(g.Rn, load3(a.R + 6)), db = matvec(g.Rn, load3(b.R + 6));   // the old optical axes in the new axes
	if (!(da.z > 0.1) || !(db.z > 0.1)) { *why = "a camera looks more than 84 degrees away from the rectified axis"; return SRH_E_UNSUPPORTED; }
	const double f = r.focal > 0 ? r.focal : (((a.K[0] + a.K[4]) + b.K[0]) + b.K[4])/4.0;
	if (!(f > 0) || !isfinite_d(f)) { *why = "no positive focal length"; return SRH_E_INVALID; }
	const double ow = (double)(r.out_w ? r.out_w : w)/image_scale, oh = (double)(r.out_h ? r.out_h : h)/image_scale;
	double cxa = ow/2 - f*da.x/da.z, cxb = ow/2 - f*db.x/db.z;
	if (r.flags & SRH_RECTIFY_SHARED_CX) cxa = cxb = (cxa + cxb)/2;
	if (!isnan_d(r.cx_a)) cxa = r.cx_a;
	if (!isnan_d(r.cx_b)) cxb = r.cx_b;
	const double cy = !isnan_d(r.cy) ? r.cy : oh/2 - f*((da.y/da.z + db.y/db.z)/2);
	for (int i = 0; i < 9; ++i) g.Ka[i] = g.Kb[i] = 0.0;
	g.Ka[0] = g.Ka[4] = g.Kb[0] = g.Kb[4] = f;
	g.Ka[2] = cxa; g.Kb[2] = cxb;
	g.Ka[5] = g.Kb[5] = cy;
	g.Ka[8] = g.Kb[8] = 1.0;
	const Vec3 ta = matvec(g.Rn, Ca), tb = matvec(g.Rn, Cb);
	g.ta[0] = -ta.x; g.ta[1] = -ta.y; g.ta[2] = -ta.z;
	g.tb[0] = -tb.x; g.tb[1] = -tb.y; g.tb[2] = -tb.z;
	return SRH_OK;
}

// the angle between a camera's optical axis and the rectified one, in radians
inline double axis_angle(const srh_camera &cam, const srh_camera &rect_cam) {
	const double c = dot(load3(cam.R + 6), load3(rect_cam.R + 6));
	return acos(c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c);
}

// ---- the warp: destination pixel (x, y) of the rectified view -> where its centre ray meets the source image, in the
// source's (scaled) pixel raster with pixel centres at integers: (u, v).  false: the point lies behind the source camera, or
// u / v is not finite -- the map holds NaN there.
// A coordinate within 1e-11*(1 + |c|) of an integer IS that integer (the round trip through two cameras leaves about 1e-14
// of noise; the parity tolerance is 1e-9): a pair that is rectified already, or any whole-pixel shift, then comes through
// byte for byte with its mask -- without it, x - 1e-14 takes the taps x - 1 and x, and the frame's mask turns ragged.
SRH_HD double warp_snap(double c) {
	const double r = floor(c + 0.5);
	return fabs(c - r) <= 1e-11*(1.0 + fabs(c)) ? r : c;
}
SRH_HD bool warp_map(const srh_camera &rect_cam, const srh_camera &src_cam, int x, int y, double s, double &u, double &v) {
	const Ray ray = cam_unproject(rect_cam, (x + 0.5)/s, (y + 0.5)/s);
	const Vec3 P = ray.src + ray.dir;
	Vec3 q = P;
	cam_project(src_cam, q);
	u = warp_snap(q.x*s - 0.5);
	v = warp_snap(q.y*s - 0.5);
	if (!(cam_local_z(src_cam, P) > 0) || !isfinite_d(u) || !isfinite_d(v)) {
		u = v = NAN;
		return false;
	}
	return true;
}

// floor(u) as an int, saturating (trunc_sat: +-2^29) -- and the weight of the tap to its right / below it
SRH_HD int warp_tap(double u, double &frac) {
	const double f = floor(u);
	frac = u - f;
	return trunc_sat(f);
}
SRH_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// one channel of the bilinear blend, rounded half up and clamped to a byte
SRH_HD uint32_t warp_blend(double a, double b, uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11) {
	const double top = (1 - a)*(double)c00 + a*(double)c10, bot = (1 - a)*(double)c01 + a*(double)c11;
	const double r = floor(top*(1 - b) + bot*b + 0.5);
	return r < 0.0 ? 0u : r > 255.0 ? 255u : (uint32_t)r;
}

// A whole destination pixel from the source planes (rgba: R | G<<8 | B<<16 | A<<24; mask: 1 = WHITE): every channel blended
// from the four taps clamped into the source; WHITE iff the taps with a weight other than 0 lie inside the source unclamped
// and are WHITE there.
SRH_HD void warp_pixel(const uint32_t *rgba, const uint8_t *mask, int sw, int sh, double u, double v, uint32_t &px, uint8_t &m) {
	double a, b;
	const int x0 = warp_tap(u, a), y0 = warp_tap(v, b);
	const int xa = clampi(x0, 0, sw - 1), xb = clampi(x0 + 1, 0, sw - 1), ya = clampi(y0, 0, sh - 1), yb = clampi(y0 + 1, 0, sh - 1);
	const size_t i00 = (size_t)ya*sw + xa, i10 = (size_t)ya*sw + xb, i01 = (size_t)yb*sw + xa, i11 = (size_t)yb*sw + xb;
	const uint32_t p00 = rgba[i00], p10 = rgba[i10], p01 = rgba[i01], p11 = rgba[i11];
	px = 0;
	for (int sh8 = 0; sh8 < 32; sh8 += 8)
		px |= warp_blend(a, b, (p00 >> sh8) & 255u, (p10 >> sh8) & 255u, (p01 >> sh8) & 255u, (p11 >> sh8) & 255u) << sh8;
	// (a tap whose weight is exactly 0 -- a == 0: the right column, b == 0: the lower row -- adds nothing to the colour and
	// is not asked for support either: a whole-pixel shift keeps its last column and row)
	const bool right = a != 0.0, below = b != 0.0;
	const bool inside = x0 >= 0 && y0 >= 0 && x0 + (right ? 1 : 0) < sw && y0 + (below ? 1 : 0) < sh;
	m = inside && mask[i00] == 1 && (!right || mask[i10] == 1) && (!below || mask[i01] == 1) && (!(right && below) || mask[i11] == 1) ? 1 : 0;
}

// ---- the way back: pixel (x, y) of the original view `dst` -> the pixel of the rectified map its centre ray falls into
// (the cross-check's pixel rule: inside the raster as doubles, then truncated), -1: behind the rectified camera or outside.
SRH_HD int64_t unrectify_index(const srh_camera &dst_cam, const srh_camera &rect_cam, int x, int y, double s, int rw, int rh, Ray &ray) {
	ray = cam_unproject(dst_cam, (x + 0.5)/s, (y + 0.5)/s);
	const Vec3 P = ray.src + ray.dir;
	Vec3 q = P;
	if (!(cam_local_z(rect_cam, P) > 0) || !cam_project(rect_cam, q)) return -1;
	const double x2 = q.x*s, y2 = q.y*s;
	if (!(x2 >= 0 && y2 >= 0 && x2 < rw && y2 < rh)) return -1;
	return (int64_t)trunc_sat(y2)*rw + trunc_sat(x2);
}

// the rectified depth dr (z along the rectified axis) on that ray, as depth in dst's camera; what is not a finite positive
// depth (+-INF, NaN, MultiViewStereo's -1) comes through unchanged
SRH_HD double unrectify_depth(const srh_camera &dst_cam, const srh_camera &rect_cam, const Ray &ray, double dr) {
	if (!isfinite_d(dr) || !(dr > 0)) return dr;
	const Vec3 X = ray.src + ray.dir*(dr / dot(load3(rect_cam.R + 6), ray.dir));
	return cam_local_z(dst_cam, X);
}

}  // namespace rect
}  // namespace srh
