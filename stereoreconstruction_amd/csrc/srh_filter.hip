// srh_filter.hip -- hole filling of one view's depth map: TwoViewStereo::filterInvalidPixels (stereo/twoviewstereo.cpp:
// 676-811, its `#if 0` half included) and weightedMedian (:821-860).  DESIGN.md 4b.
//   filter_gap_kernel     one lane per pixel: the row gap fill (srh_filter.hpp, gap_fill_pixel) from the map D into G
//   filter_holes_kernel   one lane per pixel: NaN where the mask is not WHITE, the list of WHITE non-finite pixels of D
//   filter_median_kernel  one lane per listed hole: its support window in LDS (support_window, the arithmetic of
//                         weights_kernel) and weightedMedian over G, replayed exactly (weighted_median_replay)
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_window.hpp"
#include "srh_filter.hpp"

namespace srh {

// counters (unsigned long long): [0] holes on entry, [1] pixels gap-filled, [2] holes the median made finite,
// [3] holes whose median the exact replay selected
__device__ __forceinline__ void wave_count(unsigned long long *cnt, bool pred)
{
	const unsigned long long b = __ballot(pred);
	if (b && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(cnt, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(256) void filter_gap_kernel(const double *__restrict__ D, double *__restrict__ G, int w, int h,
                                                         int gap, unsigned long long *__restrict__ cnt)
{
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	bool filled = false;
	if (q < (size_t)w*h) {
		const int x = (int)(q % w);
		double v;
		filled = filt::gap_fill_pixel(D + (q - x), w, x, gap, &v);
		G[q] = v;
	}
	wave_count(cnt + 1, filled);
}

__global__ __launch_bounds__(256) void filter_holes_kernel(const uint8_t *__restrict__ mask, double *__restrict__ D, int w, int h,
                                                           int median, uint32_t *__restrict__ holes,
                                                           unsigned long long *__restrict__ cnt)
{
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	bool hole = false;
	if (q < (size_t)w*h) {
		if (mask[q] != 1) {
			if (median) D[q] = __builtin_nan("");
		} else hole = !filt::is_fin(D[q]);
	}
	const unsigned long long b = __ballot(hole);
	if (!b) return;
	const unsigned lane = threadIdx.x & 63, first = (unsigned)(__ffsll((long long)b) - 1);
	unsigned long long base = 0;
	if (lane == first) base = atomicAdd(cnt + 0, (unsigned long long)__popcll(b));
	base = __shfl(base, (int)first);
	if (hole && median) holes[base + __popcll(b & ((1ull << lane) - 1))] = (uint32_t)q;
}

// 64 lanes, one hole each.  LDS: the lane's window (121 doubles, tap-major with a stride of 64 so that the lanes of a
// wave hit distinct banks) and its heap of tap indices (121 bytes), 70 KB a block: two blocks per CU.
#define FM_LANES 64
#define FM_TAPS 121
__global__ __launch_bounds__(FM_LANES) void filter_median_kernel(const ViewDev *__restrict__ views, int slot, srh_params P,
                                                                 const double *__restrict__ G, const uint32_t *__restrict__ holes,
                                                                 int nholes, double *__restrict__ D,
                                                                 unsigned long long *__restrict__ cnt)
{
	__shared__ double wl[FM_TAPS*FM_LANES];
	__shared__ uint8_t hp[FM_TAPS*FM_LANES];
	__shared__ int toff[FM_TAPS];
	const ViewDev &V = views[slot];
	const int W = V.w, H = V.h;
	const int R = P.window_radius, WS = 2*R + 1, T = WS*WS;
	for (int t = threadIdx.x; t < T; t += FM_LANES) toff[t] = (t / WS)*W + (t % WS);
	__syncthreads();
	const int lane = threadIdx.x;
	const int i = blockIdx.x*FM_LANES + lane;
	bool finite = false, replayed = false;
	if (i < nholes) {
		const uint32_t pix = holes[i];
		const int cx = (int)(pix % (uint32_t)W), cy = (int)(pix / (uint32_t)W);
		double *wb = wl + lane;
		support_window(V, P, cx, cy, [&](int r, int c) -> double & { return wb[(r*WS + c)*FM_LANES]; });
		// weightedMedian's keeping loop (:826-842).  The reference reads depths[PV(xt, yt)] also for taps outside the image
		// (another row, or past the map); its window weight there is exp(-geodesic_init/sigma) (adaptive: 0), which the
		// host admits only when it is not > 1e-10 (check_filter, srh_api.hip; the defaults give 0), so such a tap is never
		// kept and skipping it gives the reference's result wherever it does not fault.
		uint8_t *h = hp + lane;
		const ptrdiff_t gb = (ptrdiff_t)(cy - R)*W + (cx - R);     // G[gb + toff[t]]: tap t (in the image only)
		int n = 0;
		double total = 0.0;
		for (int row = 0; row < WS; ++row) {
			const int py = cy + row - R;
			if (py < 0 || py >= H) continue;
			for (int col = 0; col < WS; ++col) {
				const int px = cx + col - R;
				if (px < 0 || px >= W) continue;
				const int t = row*WS + col;
				const double depth = G[gb + toff[t]];
				if (filt::is_nan(depth) || depth < P.min_depth || depth > P.max_depth) continue;
				const double weight = wb[t*FM_LANES];
				if (weight > 1e-10) {
					h[n*FM_LANES] = (uint8_t)t;
					total += weight;
					++n;
				}
			}
		}
		replayed = n > 1 && total > 1e-10;
		const double ret = filt::weighted_median_replay(h, FM_LANES, n, total,
		                                                [&](uint8_t t) { return G[gb + toff[t]]; },
		                                                [&](uint8_t t) { return wb[t*FM_LANES]; });
		D[pix] = ret;
		finite = filt::is_fin(ret);
	}
	wave_count(cnt + 2, finite);
	wave_count(cnt + 3, replayed);
}

void launch_filter_gaps(hipStream_t st, const double *D, double *G, int w, int h, int gap, unsigned long long *cnt)
{
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(filter_gap_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st, D, G, w, h, gap, cnt);
}

void launch_filter_holes(hipStream_t st, const uint8_t *mask, double *D, int w, int h, bool median, uint32_t *holes,
                         unsigned long long *cnt)
{
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(filter_holes_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st, mask, D, w, h, median ? 1 : 0,
	                   holes, cnt);
}

void launch_filter_median(hipStream_t st, const ViewDev *views, int slot, const srh_params &P, const double *G,
                          const uint32_t *holes, int nholes, double *D, unsigned long long *cnt)
{
	if (nholes <= 0) return;
	hipLaunchKernelGGL(filter_median_kernel, dim3((unsigned)((nholes + FM_LANES - 1)/FM_LANES)), dim3(FM_LANES), 0, st,
	                   views, slot, P, G, holes, nholes, D, cnt);
}

}  // namespace srh
