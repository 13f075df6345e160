// rectify_host.cpp -- csrc/srh_rectify.hpp (and the camera model of csrc/srh_geom.hpp under it) compiled for the host: the
// rectifying geometry, the rig test and the warp's map, pixel by pixel as the kernels of srh_rectify.hip run them.  Built
// at test time as a shared library (tests/rectify_ref.py, lib()) and loaded with ctypes; with -DRECTIFY_HOST_MAIN it is a
// program of its own that rectifies verged pinhole rigs, warps a small image and brings a depth map back (for a run under
// -fsanitize=address,undefined on the CPU).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "srh_rectify.hpp"

extern "C" {

// out: Rn (9) | Ka (9) | Kb (9) | ta (3) | tb (3)
int rh_geometry(const srh_camera *a, const srh_camera *b, int w, int h, double scale, const srh_rectify_params *r, double *out)
{
	srh::rect::Geometry g;
	const char *why = "";
	const int rc = srh::rect::geometry(*a, *b, w, h, scale, *r, g, &why);
	if (rc) return rc;
	std::memcpy(out, g.Rn, sizeof(g.Rn));
	std::memcpy(out + 9, g.Ka, sizeof(g.Ka));
	std::memcpy(out + 18, g.Kb, sizeof(g.Kb));
	std::memcpy(out + 27, g.ta, sizeof(g.ta));
	std::memcpy(out + 30, g.tb, sizeof(g.tb));
	return 0;
}

void rh_warp_map(const srh_camera *rect_cam, const srh_camera *src_cam, int out_w, int out_h, double s, double *uv)
{
	for (int y = 0; y < out_h; ++y)
		for (int x = 0; x < out_w; ++x) {
			double u, v;
			srh::rect::warp_map(*rect_cam, *src_cam, x, y, s, u, v);
			uv[2*((size_t)y*out_w + x)] = u;
			uv[2*((size_t)y*out_w + x) + 1] = v;
		}
}

// the warp's bytes and mask for a given map (NaN: reads nothing), pixel by pixel through warp_pixel
void rh_warp_image(const uint32_t *rgba, const uint8_t *mask, int sw, int sh, const double *uv, int out_w, int out_h,
                   uint32_t *rgba_out, uint8_t *mask_out)
{
	for (size_t i = 0; i < (size_t)out_w*out_h; ++i) {
		rgba_out[i] = 0; mask_out[i] = 0;
		if (uv[2*i] == uv[2*i] && uv[2*i + 1] == uv[2*i + 1])
			srh::rect::warp_pixel(rgba, mask, sw, sh, uv[2*i], uv[2*i + 1], rgba_out[i], mask_out[i]);
	}
}

// the way back, as unrectify_kernel runs it: depth (w*h) and index (w*h) of the original view from the rectified map
void rh_unrectify(const srh_camera *dst_cam, const srh_camera *rect_cam, const uint8_t *mask, int w, int h, double s,
                  const double *depth_rect, int rw, int rh, double *depth, int32_t *index)
{
	for (int y = 0; y < h; ++y)
		for (int x = 0; x < w; ++x) {
			const size_t i = (size_t)y*w + x;
			double d = NAN;
			int64_t j = -1;
			if (mask[i] == 1) {
				srh::Ray ray;
				j = srh::rect::unrectify_index(*dst_cam, *rect_cam, x, y, s, rw, rh, ray);
				if (j >= 0) d = srh::rect::unrectify_depth(*dst_cam, *rect_cam, ray, depth_rect[j]);
			}
			depth[i] = d;
			index[i] = (int32_t)j;
		}
}

int rh_row_aligned(const srh_camera *a, const srh_camera *b)
{
	double f = 0;
	return srh::rig_is_row_aligned(*a, *b, &f) ? 1 : 0;
}

int rh_sizeof_params(void) { return (int)sizeof(srh_rectify_params); }
int rh_sizeof_info(void) { return (int)sizeof(srh_rectify_info); }

}  // extern "C"

#ifdef RECTIFY_HOST_MAIN
// a pinhole camera (no distortion, not refractive) from K = [[f, 0, cx], [0, f, cy], [0, 0, 1]], a rotation and a centre
static srh_camera pinhole(double f, double cx, double cy, const double R[9], const double Cc[3])
{
	srh_camera c;
	std::memset(&c, 0, sizeof(c));
	const double K[9] = { f, 0, cx, 0, f, cy, 0, 0, 1 }, Kinv[9] = { 1/f, 0, -cx/f, 0, 1/f, -cy/f, 0, 0, 1 };
	std::memcpy(c.K, K, sizeof(K));
	std::memcpy(c.Kinv, Kinv, sizeof(Kinv));
	std::memcpy(c.R, R, sizeof(c.R));
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) c.Rinv[i*3 + j] = R[j*3 + i];
	for (int i = 0; i < 3; ++i) { c.C[i] = Cc[i]; c.t[i] = -(R[i*3]*Cc[0] + R[i*3 + 1]*Cc[1] + R[i*3 + 2]*Cc[2]); }
	c.plane_normal[2] = 1; c.refr_index = 1;
	c.pdir[0] = R[6]; c.pdir[1] = R[7]; c.pdir[2] = R[8];
	return c;
}

static void rot_yx(double ay, double ax, double R[9])
{
	const double cy = std::cos(ay), sy = std::sin(ay), cx = std::cos(ax), sx = std::sin(ax);
	const double Ry[9] = { cy, 0, sy, 0, 1, 0, -sy, 0, cy }, Rx[9] = { 1, 0, 0, 0, cx, -sx, 0, sx, cx };
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
		double s = 0;
		for (int k = 0; k < 3; ++k) s += Rx[i*3 + k]*Ry[k*3 + j];
		R[i*3 + j] = s;
	}
}

int main()
{
	std::mt19937 rng(20240611u);
	std::uniform_real_distribution<double> U(-1.0, 1.0);
	int bad = 0, trials = 0;
	for (int trial = 0; trial < 60; ++trial) {
		const int w = 1 + (int)(rng() % 70), h = 1 + (int)(rng() % 50);
		double Ra[9], Rb[9];
		rot_yx(0.05*U(rng), 0.03*U(rng), Ra);
		rot_yx(0.05*U(rng), 0.03*U(rng), Rb);
		const double Ca[3] = { 0, 0, 0 }, Cb[3] = { 1.0, 0.05*U(rng), 0.05*U(rng) };
		const double f = w + 40.0;                        // (half a field of view below 30 degrees also for the smallest images)
		const srh_camera a = pinhole(f, w/2.0, h/2.0, Ra, Ca), b = pinhole(1.1*f, w/2.0 + 1, h/2.0 - 1, Rb, Cb);
		srh_rectify_params r;
		std::memset(&r, 0, sizeof(r));
		r.cx_a = r.cx_b = r.cy = NAN;
		r.flags = trial & 1;
		if (trial % 3 == 0) { r.out_w = w + 5; r.out_h = h + 3; }
		double g[33];
		++trials;
		if (rh_geometry(&a, &b, w, h, 1.0, &r, g)) { ++bad; continue; }
		const int ow = r.out_w ? r.out_w : w, oh = r.out_h ? r.out_h : h;
		const double Ct[3] = { Ca[0], Ca[1], Ca[2] };
		const srh_camera ra = pinhole(g[9], g[11], g[14], g, Ct), rb = pinhole(g[18], g[20], g[23], g, Cb);
		if (!rh_row_aligned(&ra, &rb) || rh_row_aligned(&a, &b)) ++bad;
		// the warp of a small image and mask, every pixel through warp_map + warp_pixel
		std::vector<uint32_t> img((size_t)w*h), out((size_t)ow*oh);
		std::vector<uint8_t> mask((size_t)w*h), mout((size_t)ow*oh);
		for (size_t i = 0; i < img.size(); ++i) { img[i] = rng(); mask[i] = rng() % 7 != 0; }
		std::vector<double> uv((size_t)ow*oh*2);
		rh_warp_map(&ra, &a, ow, oh, 1.0, uv.data());
		size_t white = 0;
		for (size_t i = 0; i < out.size(); ++i) {
			out[i] = 0; mout[i] = 0;
			if (uv[2*i] == uv[2*i]) srh::rect::warp_pixel(img.data(), mask.data(), w, h, uv[2*i], uv[2*i + 1], out[i], mout[i]);
			white += mout[i];
		}
		// far-off coordinates saturate, they do not overflow
		uint32_t px; uint8_t m;
		srh::rect::warp_pixel(img.data(), mask.data(), w, h, 1e300, -1e300, px, m);
		if (m) ++bad;
		// the way back: a constant rectified depth gives, in the original view, a finite depth wherever the index is >= 0
		std::vector<double> depth((size_t)ow*oh, 7.0);
		for (int y = 0; y < h; ++y)
			for (int x = 0; x < w; ++x) {
				srh::Ray ray;
				const int64_t j = srh::rect::unrectify_index(a, ra, x, y, 1.0, ow, oh, ray);
				if (j < -1 || j >= (int64_t)ow*oh) { ++bad; continue; }
				if (j < 0) continue;
				const double z = srh::rect::unrectify_depth(a, ra, ray, depth[(size_t)j]);
				if (!(z > 6.0 && z < 8.0)) ++bad;
				if (srh::rect::unrectify_depth(a, ra, ray, -1.0) != -1.0) ++bad;
			}
		if (w > 8 && h > 8 && white == 0) ++bad;
	}
	std::printf("rectify_host: %d findings in %d rigs\n", bad, trials);
	return bad ? 1 : 0;
}
#endif
