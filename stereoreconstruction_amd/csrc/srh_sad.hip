// srh_sad.hip -- TwoViewStereo::cost_sad (stereo/twoviewstereo.cpp:864-905), the support-weighted, truncated sum of
// absolute gray differences, as the cost of the TwoView WTA (option "cost" = SRH_COST_SAD).
//
//   sad_full_window_kernel   per pixel of the other view: is cost_sad's whole window usable there (inside, mask WHITE)?
//   twoview_rows_sad_kernel  the row-run lists' cost slots (srh_rows.hip layout), blocks of 8 adjacent columns
//   twoview_list_sad_kernel  the list-order costs (srh_list.hip layout): steep curves
//   pair_costs_kernel        the cost (any SRH_COST_* kind) of arbitrary pairs, the window built per lane (srh_twoview_pair_costs)
//
// The scans of srh_rows.hip / srh_list.hip run unchanged on these costs.  Every cost has the reference's bits: the same
// operations in the same order, a skipped tap adds +0.0 (every term is >= 0 and the sums start at +0.0).
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_window.hpp"

namespace srh {

// ------------------------------------------------------------------ fully usable windows of the other view
// cost_sad's other-view tap is right.pixel() behind rightMask: usable wherever the mask is WHITE, the last column and row
// included -- not the NCC plane `full` (gray_tv, sample() validity), and cached apart from it (ViewHost::fulls)
__global__ void sad_full_window_kernel(const uint8_t *__restrict__ mask, int W, int H, int R, uint8_t *__restrict__ full)
{
	const size_t n = (size_t)W*H;
	for (size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x*blockDim.x) {
		const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
		bool ok = x - R >= 0 && y - R >= 0 && x + R < W && y + R < H;
		for (int row = -R; ok && row <= R; ++row)
			for (int col = -R; col <= R; ++col) ok = ok && mask[(size_t)(y + row)*W + (x + col)] == 1;
		full[i] = ok ? 1 : 0;
	}
}

void launch_sad_full_window(hipStream_t st, const uint8_t *mask, int w, int h, int R, uint8_t *full) {
	size_t n = (size_t)w*h;
	size_t b = (n + 255)/256; if (b > 4096) b = 4096; if (b < 1) b = 1;
	hipLaunchKernelGGL(sad_full_window_kernel, dim3((unsigned)b), dim3(256), 0, st, mask, w, h, R, full);
}

// ------------------------------------------------------------------ row-run cost slots
// One workgroup = one wave = one wave tile of the row-run layouts: 8 adjacent pixels of an image row, 8 lanes per pixel.
// A pixel's candidates are its row spans in blocks of 8 adjacent columns (srh_rows.hip); lane g takes blocks g, g+8, ...
// A block whose 8 candidates all have a fully usable window in the other view takes the fast form: the skipped taps are
// the reference pixel's own (its per-pixel totalWeight and numPixels are constants), and a tap costs a subtraction (the
// absolute value a modifier), a minimum, a multiply and an add for each candidate -- one row segment of 8+2R values of
// the other view feeds 8 candidates x (2R+1) taps.  Any other block: the select form, every tap guarded.
#define SR_WT 8
#define SR_G 8
#define SR_NCB 8
#define SR_THREADS (SR_WT*SR_G)

template <int R>
struct SadRowsSmem {
	static constexpr int WS = 2*R + 1;
	static constexpr int WP = (WS + 1) & ~1;
	static constexpr int LW = SR_WT + 2*R;
	double w[WS][SR_WT][WP];                                   // the wave tile's windows: [window row][pixel][tap, padded]
	double lt[WS][LW];                                         // the reference rows (gray_tv: sample() behind leftMask)
	double totalW[SR_WT];                                      // fast form: totalWeight, numPixels of a fully usable other side
	int npix[SR_WT];
	int meta[SR_WT];
	uint32_t rowinfo[SR_WT][SRH_ROWS_NR];
	unsigned short blk0[SR_WT][SRH_ROWS_NR + 2];               // first 8-column block (task) of each row; [nr] = total
};

template <int R>
__global__ __launch_bounds__(SR_THREADS)
void twoview_rows_sad_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P,
                             int y0, int nrows, const double *__restrict__ wbuf, const uint8_t *__restrict__ full_oth,
                             const uint32_t *__restrict__ rowinfo, const int32_t *__restrict__ meta,
                             double *__restrict__ cost, int smax, Counters *__restrict__ cnt)
{
	constexpr int WS = 2*R + 1;
	typedef SadRowsSmem<R> Smem;
	constexpr int WP = Smem::WP;
	constexpr int NR_ = SR_NCB + 2*R;
	__shared__ Smem S;

	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w, H = L.h, OW = Rv.w, OH = Rv.h;
	const int tiles_per_row = (W + SRH_WTILE - 1)/SRH_WTILE;
	const int tid = threadIdx.x;
	const int i = tid & 7, g = tid >> 3;
	const int item = blockIdx.x;
	const int tile = item/(SRH_WTILE/SR_WT), sub = item % (SRH_WTILE/SR_WT);
	const int trow = tile / tiles_per_row;
	const int x0 = (tile % tiles_per_row)*SRH_WTILE + sub*SR_WT;
	if (x0 >= W) return;                                         // (the last tile's quarters beyond the row: the whole wave)
	const int y = y0 + trow;
	const int x = x0 + i;
	const size_t qbase = (size_t)trow*W + x0;
	double *const ctile = cost + ((size_t)trow*((W + SR_WT - 1)/SR_WT) + x0/SR_WT)*(size_t)smax*SR_WT;   // slot s of pixel pi: ctile[s*8 + pi]
	const double nan = __builtin_nan("");
	const double mcd = P.max_color_diff;
	const bool fast_ok = mcd == mcd;                           // (fmin and the reference's select agree for any non-NaN bound)

	// ---- stage: windows (band buffer in the LDS-image layout), reference rows, row tables
	{
		const double *wt = wbuf + wimg_offset(W, R, trow, x0);
		for (int idx = tid; idx < WS*SR_WT*WP; idx += SR_THREADS) {
			const int a = idx/(SR_WT*WP), rest = idx % (SR_WT*WP);
			S.w[a][rest/WP][rest % WP] = wt[(size_t)a*wimg_row_stride(R) + rest];
		}
		for (int idx = tid; idx < WS*Smem::LW; idx += SR_THREADS) {
			const int ty = idx / Smem::LW, tx = idx % Smem::LW;
			const int gx = x0 - R + tx, gy = y - R + ty;
			S.lt[ty][tx] = (gx >= 0 && gy >= 0 && gx < W && gy < H) ? L.gray_tv[(size_t)gy*W + gx] : nan;
		}
		for (int idx = tid; idx < SR_WT*SRH_ROWS_NR; idx += SR_THREADS) {
			const int pi = idx / SRH_ROWS_NR;
			const size_t qq = qbase + pi;
			S.rowinfo[pi][idx % SRH_ROWS_NR] = (x0 + pi < W) ? rowinfo[((qq >> 6)*SRH_ROWS_NR + idx % SRH_ROWS_NR)*64 + (qq & 63)] : 0u;
		}
		if (tid < SR_WT) S.meta[tid] = (x0 + tid < W) ? meta[qbase + tid] : 0;
	}
	__syncthreads();

	// ---- per-pixel constants of the fast form (one lane per pixel): the reference's totalWeight and numPixels when every
	// tap of the other side is usable -- the same additions in the same order (a skipped tap adds +0.0)
	if (g == 0) {
		double tw = 0.0;
		int np = 0;
		for (int row = 0; row < WS; ++row)
			for (int col = 0; col < WS; ++col) {
				const double gl = S.lt[row][i + col], wt = S.w[row][i][col];
				const bool okl = gl == gl && wt > P.weight_cutoff;
				tw += okl ? wt : 0.0;
				np += okl ? 1 : 0;
			}
		S.totalW[i] = tw; S.npix[i] = np;
		const int nr = (x < W) ? S.meta[i] >> 16 : 0;
		int nblk = 0;
		for (int r = 0; r < nr; ++r) {
			S.blk0[i][r] = (unsigned short)nblk;
			nblk += ((int)(S.rowinfo[i][r] >> 16) + SR_NCB - 1)/SR_NCB;
		}
		S.blk0[i][nr] = (unsigned short)nblk;
	}
	__syncthreads();

	unsigned n_dev = 0;
	if (x < W) {
		const int m = S.meta[i];
		const int ymin = (int)(short)(m & 0xffff), nr = m >> 16;
		double *const crow = ctile + i;
		const double tw_full = S.totalW[i];
		const bool bad_full = S.npix[i] <= 4 || tw_full <= 1e-10;
		const int ntask = S.blk0[i][nr];
		int r = 0;
		for (int task = g; task < ntask; task += SR_G) {
			while (task >= (int)S.blk0[i][r + 1]) ++r;
			const uint32_t info = S.rowinfo[i][r];
			const int xlo = (int)(short)(info & 0xffff), wdt = (int)(info >> 16);
			const int b = task - (int)S.blk0[i][r];
			const int cy = ymin + r;
			const int c0 = xlo + b*SR_NCB;
			const int nv = wdt - b*SR_NCB < SR_NCB ? wdt - b*SR_NCB : SR_NCB;
			n_dev += nv;
			double *const dst = crow + (size_t)task*SR_NCB*SR_WT;
			// (a span's candidates lie inside the other image; so do their windows when `full` says so)
			bool fast = fast_ok;
			for (int j = 0; j < nv; ++j) fast = fast && full_oth[(size_t)cy*OW + c0 + j] != 0;
			if (fast) {
				// the columns right of a partial block's last candidate are read clamped and their sums dropped
				double acc[SR_NCB];
#pragma unroll
				for (int j = 0; j < SR_NCB; ++j) acc[j] = 0.0;
#pragma unroll 1
				for (int row = 0; row < WS; ++row) {
					const double *rp = Rv.gray + (size_t)(cy - R + row)*OW;
					double rr[NR_];
#pragma unroll
					for (int k = 0; k < NR_; ++k) {
						int gx = c0 - R + k;
						gx = gx < OW ? gx : OW - 1;
						rr[k] = rp[gx];
					}
#pragma unroll
					for (int col = 0; col < WS; ++col) {
						const double gl = S.lt[row][i + col], wt = S.w[row][i][col];
						const bool okl = gl == gl && wt > P.weight_cutoff;
						const double we = okl ? wt : 0.0, g0 = okl ? gl : 0.0;   // a skipped tap: 0 * min(|0 - r|, MAX) = +0.0
#pragma unroll
						for (int j = 0; j < SR_NCB; ++j) acc[j] += we*__builtin_fmin(fabs(g0 - rr[col + j]), mcd);
					}
				}
#pragma unroll
				for (int j = 0; j < SR_NCB; ++j)
					if (j < nv) dst[j*SR_WT] = bad_full ? P.bad_ret : acc[j] / tw_full;
			} else {
				double s[SR_NCB], t[SR_NCB];
				int np[SR_NCB];
#pragma unroll
				for (int j = 0; j < SR_NCB; ++j) { s[j] = 0.0; t[j] = 0.0; np[j] = 0; }
#pragma unroll 1
				for (int row = 0; row < WS; ++row) {
					const int gy = cy - R + row;
					const bool rowok = gy >= 0 && gy < OH;
					const size_t rbase = (size_t)(rowok ? gy : 0)*OW;
					double rr[NR_];
					bool rv[NR_];
#pragma unroll
					for (int k = 0; k < NR_; ++k) {
						const int gx = c0 - R + k;
						const bool in = rowok && gx >= 0 && gx < OW;
						const size_t at = rbase + (in ? gx : 0);
						rv[k] = in && Rv.mask[at] == 1;
						rr[k] = rv[k] ? Rv.gray[at] : 0.0;
					}
#pragma unroll
					for (int col = 0; col < WS; ++col) {
						const double gl = S.lt[row][i + col], wt = S.w[row][i][col];
						const bool okl = gl == gl && wt > P.weight_cutoff;
#pragma unroll
						for (int j = 0; j < SR_NCB; ++j) {
							const bool ok = okl && rv[col + j];
							const double diff = fabs(gl - rr[col + j]);
							const double term = wt*(diff < mcd ? diff : mcd);
							s[j] += ok ? term : 0.0;
							t[j] += ok ? wt : 0.0;
							np[j] += ok ? 1 : 0;
						}
					}
				}
#pragma unroll
				for (int j = 0; j < SR_NCB; ++j)
					if (j < nv) dst[j*SR_WT] = (np[j] <= 4 || t[j] <= 1e-10) ? P.bad_ret : s[j] / t[j];
			}
		}
	}
	block_count_add(&cnt->n_eval_device, n_dev);
}

bool launch_twoview_rows_sad(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                             int y0, int nrows, const double *wbuf, const uint8_t *full_sad_oth,
                             const uint32_t *rowinfo, const int32_t *meta, double *cost, int smax, Counters *cnt)
{
	const size_t items = (size_t)((width + SRH_WTILE - 1)/SRH_WTILE)*(SRH_WTILE/SR_WT)*nrows;
	const dim3 grid((unsigned)items);
#define SRH_RS(RR) case RR: hipLaunchKernelGGL(twoview_rows_sad_kernel<RR>, grid, dim3(SR_THREADS), 0, st, views, ref, oth, P, \
	                                           y0, nrows, wbuf, full_sad_oth, rowinfo, meta, cost, smax, cnt); return true;
	switch (P.window_radius) { SRH_RS(1) SRH_RS(2) SRH_RS(3) SRH_RS(4) SRH_RS(5) default: return false; }
#undef SRH_RS
}

// ------------------------------------------------------------------ list-order costs
// steep curves (list_mode 2): one wave per reference pixel, a lane per list entry, tv_cost_sad on the tile-major window
// (the wave's lanes read the same taps: one broadcast load each)
__global__ __launch_bounds__(64)
void twoview_list_sad_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P,
                             int y0, int nrows, const double *__restrict__ wbuf, const int32_t *__restrict__ count,
                             const uint32_t *__restrict__ cand, double *__restrict__ cost, int cmax, Counters *__restrict__ cnt)
{
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w;
	const size_t q = blockIdx.x;
	const int x = (int)(q % W), trow = (int)(q / W), y = y0 + trow;
	unsigned n_dev = 0;
	if (L.mask[(size_t)y*W + x] == 1) {
		const int T = (2*P.window_radius + 1)*(2*P.window_radius + 1);
		const double *wq = wbuf + wbuf_offset(W, T, trow, x);
		const int n = count[q] < cmax ? count[q] : cmax;
		for (int k = threadIdx.x; k < n; k += 64) {
			const uint32_t e = cand[q*(size_t)cmax + k];
			cost[q*(size_t)cmax + k] = tv_cost_sad(L, Rv, wq, SRH_WTILE, P, x, y, (int)(e & 0xffffu), (int)(e >> 16));
			++n_dev;
		}
	}
	block_count_add(&cnt->n_eval_device, n_dev);
}

void launch_twoview_list_sad(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                             int y0, int nrows, const double *wbuf, const int32_t *count, const uint32_t *cand,
                             double *cost, int cmax, Counters *cnt)
{
	const size_t n = (size_t)nrows*width;
	hipLaunchKernelGGL(twoview_list_sad_kernel, dim3((unsigned)n), dim3(64), 0, st,
	                   views, ref, oth, P, y0, nrows, wbuf, count, cand, cost, cmax, cnt);
}

// ------------------------------------------------------------------ arbitrary pairs
// 64 lanes, one pair each; the lane's window of (x1, y1) in LDS, tap-major with a stride of 64 (support_window: the bits
// of weights_kernel), then the reference-form cost.  (x1, y1) lies inside the reference view (the caller checks).
#define PC_LANES 64
#define PC_TAPS 121
__global__ __launch_bounds__(PC_LANES)
void pair_costs_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P, int kind, int n,
                       const int32_t *__restrict__ xy, double *__restrict__ out)
{
	__shared__ double wl[PC_TAPS*PC_LANES];
	const int lane = threadIdx.x;
	const int k = blockIdx.x*PC_LANES + lane;
	if (k >= n) return;
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int x1 = xy[4*k], y1 = xy[4*k + 1], x2 = xy[4*k + 2], y2 = xy[4*k + 3];
	const int WS = 2*P.window_radius + 1;
	double *wb = wl + lane;
	support_window(L, P, x1, y1, [&](int r, int c) -> double & { return wb[(r*WS + c)*PC_LANES]; });
	out[k] = tv_cost_of(kind, L, Rv, wb, PC_LANES, P, x1, y1, x2, y2);
}

void launch_pair_costs(hipStream_t st, const ViewDev *views, int ref, int oth, const srh_params &P, int kind, int n,
                       const int32_t *xy, double *out)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(pair_costs_kernel, dim3((unsigned)((n + PC_LANES - 1)/PC_LANES)), dim3(PC_LANES), 0, st,
	                   views, ref, oth, P, kind, n, xy, out);
}

} // namespace srh
