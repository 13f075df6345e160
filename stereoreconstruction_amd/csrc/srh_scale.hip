// srh_scale.hip -- the image scaling at the top of the reference's path, on the device, in Qt 5.9.7's arithmetic
// (DESIGN.md 4f): what MultiViewStereo::initialize (multiviewstereo.cpp:216-241) and TwoViewStereo's constructor
// (twoviewstereo.cpp:89-124) get from QImage::scaledToWidth before anything else runs.
//   premultiply_kernel     Format_ARGB32 -> Format_ARGB32_Premultiplied in place (an opaque source: alpha := 255)
//   smooth_scale_kernel    Qt::SmoothTransformation, strict downscale in both axes
//   fast_scale_kernel      Qt::FastTransformation (the source of MultiViewStereo's mask)
//   scale_mask_kernel      the mask bytes of a slot from a scaled image
// All integer.  tests/qt_scale_ref.py restates the same arithmetic in numpy and is held to the installed Qt byte for byte
// (tests/test_qt_scale_restatement.py); tests/test_gpu_scale.py holds these kernels to it.
// Pixels are the words of srh_internal.hpp: R | G<<8 | B<<16 | A<<24.  Qt's words keep B and R the other way round; every
// rule here treats the three colour bytes alike, so the order does not matter.
#include "srh_internal.hpp"

#include <cmath>

namespace srh {

// ------------------------------------------------------------------ sizes (host)
// dw = (int)(sw*scale), the truncation of the reference's call; f = dw/sw; smooth: dh = (int)(f*sh + 0.9999), fast:
// dh = floor(f*sh + 0.5) (QImage::transformed).  Returns SRH_OK, or the code of the refusal with *why set.
int scale_target_size(int sw, int sh, double scale, int mode, int *dw_out, int *dh_out, const char **why) {
	*why = "";
	if (sw <= 0 || sh <= 0) { *why = "empty source image"; return SRH_E_INVALID; }
	if (mode != SRH_SCALE_SMOOTH && mode != SRH_SCALE_FAST) { *why = "unknown scaling mode"; return SRH_E_INVALID; }
	const double t = (double)sw*scale;
	if (!(t > -2147483648.0 && t < 2147483648.0)) { *why = "image_scale out of range"; return SRH_E_INVALID; }
	const int dw = (int)t;
	if (dw <= 0) { *why = "the scaled width is not positive"; return SRH_E_INVALID; }
	if (dw == sw) { *dw_out = sw; *dh_out = sh; return SRH_OK; }          // Qt returns the image itself
	if (dw > sw) { *why = "up-scaling is not restated"; return SRH_E_UNSUPPORTED; }
	const double f = (double)dw/(double)sw;
	const int dh = mode == SRH_SCALE_SMOOTH ? (int)(f*sh + 0.9999) : (int)std::floor(f*sh + 0.5);
	if (dh <= 0) { *why = "the scaled height is not positive"; return SRH_E_INVALID; }
	if (dh >= sh) { *why = "not a strict downscale in both axes"; return SRH_E_UNSUPPORTED; }
	*dw_out = dw; *dh_out = dh;
	return SRH_OK;
}

// ------------------------------------------------------------------ the smooth scale's taps
// One axis scaled down from s to d: inc = (s<<16)/d, Cp = ((d<<14) + s - 1)/s.  Target index i starts at tap p = (i*inc)>>16
// with weight ap = ((0x10000 - (i*inc & 0xffff))*Cp)>>16, goes on with weight Cp while more than Cp of the 1<<14 is left,
// and ends on one tap with the rest: n taps, the last of weight `last` in (0, Cp].
struct AxisTap { int p, n, ap, last; };
__host__ __device__ inline AxisTap axis_tap(int i, long long inc, int cp) {
	const long long val = (long long)i*inc;
	AxisTap t;
	t.p = (int)(val >> 16);
	t.ap = (int)(((0x10000 - (val & 0xffff))*cp) >> 16);
	const int j = (1 << 14) - t.ap;                                     // > 0: ap <= Cp <= 1<<14 - 1 for d < s
	const int mid = (j - 1)/cp;
	t.last = j - mid*cp;
	t.n = mid + 2;
	return t;
}
__host__ __device__ inline uint32_t tap_weight(const AxisTap &t, int k, int cp) {
	return (uint32_t)(k == 0 ? t.ap : (k == t.n - 1 ? t.last : cp));
}
void scale_axis_constants(int s, int d, long long *inc, int *cp) {
	*inc = ((long long)s << 16)/d;
	*cp = (int)((((long long)d << 14) + s - 1)/s);
}
// the last tap of every run lies inside the axis (the kernel clamps its staging to the image as well)
bool scale_axis_inside(int s, int d) {
	long long inc; int cp;
	scale_axis_constants(s, d, &inc, &cp);
	for (int i = 0; i < d; ++i) { const AxisTap t = axis_tap(i, inc, cp); if (t.p < 0 || t.p + t.n > s) return false; }
	return true;
}

// ------------------------------------------------------------------ the fast scale's index maps (host)
// Qt 5.9 draws the source through a QPainter with the scale set.  An image with alpha (Format_ARGB32) takes the raster
// engine's span path: the inverse of translate(1/65536) * scale(f) applied in doubles at the centre of the first pixel of
// every span piece (a target row in pieces of 2048 pixels), then stepped along x in 16.16 fixed point -- rows are placed in
// doubles one by one, columns by an integer step.  An image without alpha (Format_RGB32) takes the integer blitter, which
// steps both axes in 16.16 fixed point.  The doubles are Qt's own operations in Qt's order (x86-64, no contraction); this
// file is built with -ffp-contract=off.  map: dw column indices, then dh row indices; false: an index left the image.
bool scale_fast_maps(int sw, int sh, int dw, int dh, bool has_alpha, int32_t *map) {
	const double f = (double)dw/(double)sw;
	int32_t *xs = map, *ys = map + dw;
	if (has_alpha) {
		const double inv = 1.0/f;
		const double off = -((1.0/65536.0)*f)*inv;
		const int step = (int)(inv*65536.0);
		int fx = 0;
		for (int i = 0; i < dw; ++i) {
			if (i % 2048 == 0) fx = (int)((inv*(i + 0.5) + off)*65536.0);
			xs[i] = fx >> 16;
			fx += step;
		}
		for (int j = 0; j < dh; ++j) ys[j] = (int)((inv*(j + 0.5) + off)*65536.0) >> 16;
	} else {
		for (int axis = 0; axis < 2; ++axis) {
			const int s = axis ? sh : sw, d = axis ? dh : dw;
			const double sc = (f*s)/s;                                      // target extent / source extent, as the blitter forms it
			const long long m = (long long)(int)(65536.0/sc);
			const long long first = (long long)std::ceil(0.5*(double)m) - 1;
			for (int i = 0; i < d; ++i) (axis ? ys : xs)[i] = (int32_t)((first + m*i) >> 16);
		}
	}
	for (int i = 0; i < dw; ++i) if (xs[i] < 0 || xs[i] >= sw) return false;
	for (int j = 0; j < dh; ++j) if (ys[j] < 0 || ys[j] >= sh) return false;
	return true;
}

// ------------------------------------------------------------------ kernels
static inline int scale_grid(size_t n) {
	size_t b = (n + 255)/256;
	return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// Qt's premultiplication, two channels per multiplication: t = (x & 0xff00ff)*a; t = (t + ((t>>8) & 0xff00ff) + 0x800080)>>8
__global__ void premultiply_kernel(uint32_t *__restrict__ px, size_t n, int has_alpha) {
	for (size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x*blockDim.x) {
		uint32_t x = px[i];
		if (!has_alpha) { px[i] = x | 0xff000000u; continue; }
		const uint32_t a = x >> 24;
		uint32_t t = (x & 0xff00ffu)*a;
		t = (t + ((t >> 8) & 0xff00ffu) + 0x800080u) >> 8;
		t &= 0xff00ffu;
		// green by the same pair form, with alpha as its idle partner (a*a << 16 fits the word and carries nothing down): the
		// single-channel form x = g*a; x += ((x >> 8) & 0xff) + 0x80 is the same number, but hipcc 7.2 -O3 turns it into a
		// v_dot4_u32_u8 that computes 2*g*a + 8 (seen in the ISA and on the device)
		uint32_t u = ((x >> 8) & 0xff00ffu)*a;
		u = (u + ((u >> 8) & 0xff00ffu) + 0x800080u) >> 8;
		px[i] = ((u & 0xffu) << 8) | t | (a << 24);
	}
}

// A workgroup makes a tile of SC_TW x SC_TH target pixels.  The source rows of the tile go by in chunks of SC_RB rows: each
// wave takes a row, stages the piece of it the tile's columns read in LDS with 16-byte loads (in pieces of SC_XC pixels),
// and every lane forms the horizontal run sum of its target column ONCE for that source row -- into H, shifted right by 4;
// then every thread adds what the chunk holds of the vertical runs of its two target pixels, in registers, in unsigned
// 32-bit arithmetic.  A pixel's channel is its total >> 24.  Any ratio works: a run longer than a piece or a chunk is
// summed over several.  src: 16-byte aligned, readable up to 3 pixels past its end (the aligned loads of the last row).
#define SC_TW 64
#define SC_TH 8
#define SC_RB 40
#define SC_XC 1024
__global__ __launch_bounds__(256) void smooth_scale_kernel(const uint32_t *__restrict__ src, int sw, int sh,
                                                           uint32_t *__restrict__ dst, int dw, int dh,
                                                           long long xinc, int xcp, long long yinc, int ycp)
{
	__shared__ uint4 H[SC_RB][SC_TW];
	__shared__ uint4 stage[4][SC_XC/4 + 1];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int x0 = blockIdx.x*SC_TW, y0 = blockIdx.y*SC_TH;
	const int nx = min(SC_TW, dw - x0), ny = min(SC_TH, dh - y0);
	const bool colok = lane < nx;
	const AxisTap cx = axis_tap(x0 + (colok ? lane : 0), xinc, xcp);
	const AxisTap cl = axis_tap(x0 + nx - 1, xinc, xcp), rl = axis_tap(y0 + ny - 1, yinc, ycp);
	const int sx0 = axis_tap(x0, xinc, xcp).p, sx1 = min(cl.p + cl.n, sw);     // source columns and rows of the tile
	const int sy0 = axis_tap(y0, yinc, ycp).p, sy1 = min(rl.p + rl.n, sh);
	AxisTap ry[2];
	bool rowok[2];
	uint32_t acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
	for (int q = 0; q < 2; ++q) {
		rowok[q] = colok && wave + 4*q < ny;
		ry[q] = axis_tap(y0 + (rowok[q] ? wave + 4*q : 0), yinc, ycp);
	}
	for (int rb = sy0; rb < sy1; rb += SC_RB) {
		const int nr = min(SC_RB, sy1 - rb);
		for (int r0 = 0; r0 < nr; r0 += 4) {                            // (block-uniform trip counts: the barriers below)
			const int r = r0 + wave;
			const bool live = r < nr;
			uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
			for (int cb = sx0; cb < sx1; cb += SC_XC) {
				const int ce = min(cb + SC_XC, sx1);
				const size_t g = (size_t)(rb + (live ? r : 0))*sw + cb, g4 = g & ~(size_t)3;
				const int shift = (int)(g - g4);
				if (live) {
					const int nvec = (shift + (ce - cb) + 3) >> 2;          // <= SC_XC/4 + 1
					const uint4 *gp = reinterpret_cast<const uint4 *>(src + g4);
					for (int v = lane; v < nvec; v += 64) stage[wave][v] = gp[v];
				}
				__syncthreads();
				if (live && colok) {
					const uint32_t *sp = reinterpret_cast<const uint32_t *>(stage[wave]) + shift - cb;   // sp[x]: pixel x of the row
					const int k0 = max(cx.p, cb) - cx.p, k1 = min(cx.p + cx.n, ce) - cx.p;
					for (int k = k0; k < k1; ++k) {
						const uint32_t px = sp[cx.p + k], w = tap_weight(cx, k, xcp);
						s0 += (px & 255u)*w; s1 += ((px >> 8) & 255u)*w; s2 += ((px >> 16) & 255u)*w; s3 += (px >> 24)*w;
					}
				}
				__syncthreads();
			}
			if (live && colok) H[r][lane] = make_uint4(s0 >> 4, s1 >> 4, s2 >> 4, s3 >> 4);
		}
		__syncthreads();
		for (int q = 0; q < 2; ++q) {
			if (!rowok[q]) continue;
			const int k0 = max(ry[q].p, rb) - ry[q].p, k1 = min(ry[q].p + ry[q].n, rb + nr) - ry[q].p;
			for (int k = k0; k < k1; ++k) {
				const uint4 hv = H[ry[q].p + k - rb][lane];
				const uint32_t w = tap_weight(ry[q], k, ycp);
				acc[q][0] += hv.x*w; acc[q][1] += hv.y*w; acc[q][2] += hv.z*w; acc[q][3] += hv.w*w;
			}
		}
		__syncthreads();
	}
	for (int q = 0; q < 2; ++q)
		if (rowok[q])
			dst[(size_t)(y0 + wave + 4*q)*dw + x0 + lane] =
				(acc[q][0] >> 24) | ((acc[q][1] >> 24) << 8) | ((acc[q][2] >> 24) << 16) | ((acc[q][3] >> 24) << 24);
}

// map: dw source columns, then dh source rows (scale_fast_maps).  With alpha a fully transparent pixel comes out as zero
// (the painter skips it over the zero-filled target); without, alpha is 255.
__global__ void fast_scale_kernel(const uint32_t *__restrict__ src, int sw, uint32_t *__restrict__ dst, int dw, int dh,
                                  const int32_t *__restrict__ map, int has_alpha)
{
	const size_t n = (size_t)dw*dh;
	for (size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x*blockDim.x) {
		const int x = (int)(i % (size_t)dw), y = (int)(i / (size_t)dw);
		const uint32_t px = src[(size_t)map[dw + y]*sw + map[x]];
		dst[i] = has_alpha ? ((px >> 24) ? px : 0u) : (px | 0xff000000u);
	}
}

// mask of a w x h view from an mw x mh scaled image: alpha_only: WHITE <=> alpha == 255 (MultiViewStereo's fast-scaled copy),
// else WHITE <=> r = g = b = a = 255 (TwoViewStereo's mask image); pixels beyond the image are not WHITE
__global__ void scale_mask_kernel(const uint32_t *__restrict__ img, int mw, int mh, int alpha_only,
                                  uint8_t *__restrict__ mask, int w, int h)
{
	const size_t n = (size_t)w*h;
	for (size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x*blockDim.x) {
		const int x = (int)(i % (size_t)w), y = (int)(i / (size_t)w);
		uint8_t m = 0;
		if (x < mw && y < mh) {
			const uint32_t px = img[(size_t)y*mw + x];
			m = alpha_only ? (px >> 24) == 255u : px == 0xffffffffu;
		}
		mask[i] = m;
	}
}

void launch_premultiply(hipStream_t st, uint32_t *px, size_t n, bool has_alpha) {
	hipLaunchKernelGGL(premultiply_kernel, dim3(scale_grid(n)), dim3(256), 0, st, px, n, has_alpha ? 1 : 0);
}

void launch_smooth_scale(hipStream_t st, const uint32_t *src, int sw, int sh, uint32_t *dst, int dw, int dh) {
	long long xinc, yinc; int xcp, ycp;
	scale_axis_constants(sw, dw, &xinc, &xcp);
	scale_axis_constants(sh, dh, &yinc, &ycp);
	hipLaunchKernelGGL(smooth_scale_kernel, dim3((dw + SC_TW - 1)/SC_TW, (dh + SC_TH - 1)/SC_TH), dim3(256), 0, st,
	                   src, sw, sh, dst, dw, dh, xinc, xcp, yinc, ycp);
}

void launch_fast_scale(hipStream_t st, const uint32_t *src, int sw, uint32_t *dst, int dw, int dh, const int32_t *map, bool has_alpha) {
	hipLaunchKernelGGL(fast_scale_kernel, dim3(scale_grid((size_t)dw*dh)), dim3(256), 0, st, src, sw, dst, dw, dh, map, has_alpha ? 1 : 0);
}

void launch_scale_mask(hipStream_t st, const uint32_t *img, int mw, int mh, bool alpha_only, uint8_t *mask, int w, int h) {
	hipLaunchKernelGGL(scale_mask_kernel, dim3(scale_grid((size_t)w*h)), dim3(256), 0, st, img, mw, mh, alpha_only ? 1 : 0, mask, w, h);
}

} // namespace srh
