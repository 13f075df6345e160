// srh_census.hip -- the support-weighted census cost of the TwoView WTA (option "cost" = SRH_COST_CENSUS).
// Not in the reference: cost_sad's tap rule, totalWeight, numPixels and bad_ret rule with the per-tap term replaced by the
// Hamming distance of two 9x7 census signatures.
//
//   census_kernel               a view's signature plane from its gray plane (one uint64_t per pixel)
//   twoview_rows_census_kernel  the row-run lists' cost slots (srh_rows.hip layout), blocks of 8 adjacent columns
//   twoview_list_census_kernel  the list-order costs (srh_list.hip layout): steep curves
//
// The scans of srh_rows.hip / srh_list.hip run unchanged on these costs.  Every cost has the bits of tv_cost_census
// (srh_walk.hpp): the same fused multiply-adds in the same order, a skipped tap carries the weight +0.0 and leaves the
// sums as they are (every term is >= 0 and the sums start at +0.0) -- the argument of srh_sad.hip.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_window.hpp"

namespace srh {

// ------------------------------------------------------------------ signatures
// Bit k = (dy + 3)*9 + (dx + 4), dy in -3..3, dx in -4..4: set iff the neighbour is inside the image and darker than the
// centre.  The centre's own bit (31) and bit 63 stay 0.  A tile of 32 x 8 pixels with its halo of 4 columns and 3 rows in
// LDS; a position outside the image holds NaN, which is darker than nothing.
#define CS_TW 32
#define CS_TH 8
#define CS_HX 4
#define CS_HY 3
__global__ __launch_bounds__(CS_TW*CS_TH)
void census_kernel(const double *__restrict__ gray, int W, int H, uint64_t *__restrict__ out)
{
	__shared__ double t[CS_TH + 2*CS_HY][CS_TW + 2*CS_HX];
	const int tiles_x = (W + CS_TW - 1)/CS_TW;
	const int bx = (int)(blockIdx.x % (unsigned)tiles_x)*CS_TW, by = (int)(blockIdx.x / (unsigned)tiles_x)*CS_TH;
	const int tid = threadIdx.x;
	for (int idx = tid; idx < (CS_TH + 2*CS_HY)*(CS_TW + 2*CS_HX); idx += CS_TW*CS_TH) {
		const int ty = idx / (CS_TW + 2*CS_HX), tx = idx % (CS_TW + 2*CS_HX);
		const int gx = bx - CS_HX + tx, gy = by - CS_HY + ty;
		t[ty][tx] = (gx >= 0 && gy >= 0 && gx < W && gy < H) ? gray[(size_t)gy*W + gx] : __builtin_nan("");
	}
	__syncthreads();
	const int lx = tid % CS_TW, ly = tid / CS_TW;
	const int x = bx + lx, y = by + ly;
	if (x >= W || y >= H) return;
	const double c = t[ly + CS_HY][lx + CS_HX];
	uint32_t lo = 0, hi = 0;                                     // bits 0..31 and 32..63 (two halves: 32-bit integer work)
#pragma unroll
	for (int dy = -CS_HY; dy <= CS_HY; ++dy)
#pragma unroll
		for (int dx = -CS_HX; dx <= CS_HX; ++dx) {
			const int k = (dy + CS_HY)*(2*CS_HX + 1) + (dx + CS_HX);
			if (dy == 0 && dx == 0) continue;
			const uint32_t b = t[ly + CS_HY + dy][lx + CS_HX + dx] < c ? 1u : 0u;
			if (k < 32) lo |= b << k; else hi |= b << (k - 32);
		}
	out[(size_t)y*W + x] = (uint64_t)lo | ((uint64_t)hi << 32);
}

void launch_census(hipStream_t st, const double *gray, int w, int h, uint64_t *out) {
	const unsigned tiles = (unsigned)((w + CS_TW - 1)/CS_TW)*(unsigned)((h + CS_TH - 1)/CS_TH);
	hipLaunchKernelGGL(census_kernel, dim3(tiles), dim3(CS_TW*CS_TH), 0, st, gray, w, h, out);
}

// ------------------------------------------------------------------ row-run cost slots
// Layout and task split of twoview_rows_sad_kernel (srh_sad.hip): one workgroup = one wave = 8 adjacent pixels of an image
// row, 8 lanes per pixel; a pixel's candidates are its row spans in blocks of 8 adjacent columns, lane g takes blocks g,
// g + 8, ...  The reference side is settled once per tile in LDS: a tap the reference pixel skips (gray_tv NaN, weight at
// or below the cut-off) gets the weight +0.0, and the reference signatures sit beside the weights.  A block whose 8
// candidates all have a fully usable window in the other view (ViewHost::fulls, cost_sad's plane) takes the fast form: one
// row segment of 8 + 2R signatures of the other view feeds 8 candidates x (2R + 1) taps, a tap costs two XORs, two
// population counts, a convert and one FP64 multiply-add per candidate; totalWeight and numPixels are the reference
// pixel's constants.  Any other block: the select form, every tap guarded.
#define CR_WT 8
#define CR_G 8
#define CR_NCB 8
#define CR_THREADS (CR_WT*CR_G)

template <int R>
struct CensusRowsSmem {
	static constexpr int WS = 2*R + 1;
	static constexpr int WP = (WS + 1) & ~1;
	static constexpr int LW = CR_WT + 2*R;
	double w[WS][CR_WT][WP];                                   // the wave tile's windows, settled: [window row][pixel][tap, padded]
	uint64_t sl[WS][LW];                                       // the reference rows' signatures (0 outside the image: never counted)
	double lt[WS][LW];                                         // the reference rows' gray_tv (settling only)
	double totalW[CR_WT];                                      // fast form: totalWeight, numPixels of a fully usable other side
	int npix[CR_WT];
	int meta[CR_WT];
	unsigned short okl[WS][CR_WT];                             // bit col: the reference side counts tap (row, col) (select form's numPixels)
	uint32_t rowinfo[CR_WT][SRH_ROWS_NR];
	unsigned short blk0[CR_WT][SRH_ROWS_NR + 2];               // first 8-column block (task) of each row; [nr] = total
};

__device__ __forceinline__ double census_term(uint64_t a, uint64_t b) {
	return (double)__builtin_popcountll(a ^ b);
}

// (3 waves per SIMD, the row-run SAD kernel's occupancy: without the bound the r = 4 and r = 5 instantiations take 171 and 182
// VGPRs, one wave less; with it 167, no scratch -- profiles/census_resources.txt)
template <int R>
__global__ __launch_bounds__(CR_THREADS, 3)
void twoview_rows_census_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P,
                                int y0, int nrows, const double *__restrict__ wbuf, const uint8_t *__restrict__ full_oth,
                                const uint32_t *__restrict__ rowinfo, const int32_t *__restrict__ meta,
                                double *__restrict__ cost, int smax, Counters *__restrict__ cnt)
{
	constexpr int WS = 2*R + 1;
	typedef CensusRowsSmem<R> Smem;
	constexpr int WP = Smem::WP;
	constexpr int NR_ = CR_NCB + 2*R;
	__shared__ Smem S;

	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w, H = L.h, OW = Rv.w, OH = Rv.h;
	const int tiles_per_row = (W + SRH_WTILE - 1)/SRH_WTILE;
	const int tid = threadIdx.x;
	const int i = tid & 7, g = tid >> 3;
	const int item = blockIdx.x;
	const int tile = item/(SRH_WTILE/CR_WT), sub = item % (SRH_WTILE/CR_WT);
	const int trow = tile / tiles_per_row;
	const int x0 = (tile % tiles_per_row)*SRH_WTILE + sub*CR_WT;
	if (x0 >= W) return;                                         // (the last tile's quarters beyond the row: the whole wave)
	const int y = y0 + trow;
	const int x = x0 + i;
	const size_t qbase = (size_t)trow*W + x0;
	double *const ctile = cost + ((size_t)trow*((W + CR_WT - 1)/CR_WT) + x0/CR_WT)*(size_t)smax*CR_WT;   // slot s of pixel pi: ctile[s*8 + pi]
	const uint64_t *__restrict__ const csL = L.census;
	const uint64_t *__restrict__ const csR = Rv.census;

	// ---- stage: windows (band buffer in the LDS-image layout), reference rows and their signatures, row tables
	{
		const double *wt = wbuf + wimg_offset(W, R, trow, x0);
		for (int idx = tid; idx < WS*CR_WT*WP; idx += CR_THREADS) {
			const int a = idx/(CR_WT*WP), rest = idx % (CR_WT*WP);
			S.w[a][rest/WP][rest % WP] = wt[(size_t)a*wimg_row_stride(R) + rest];
		}
		for (int idx = tid; idx < WS*Smem::LW; idx += CR_THREADS) {
			const int ty = idx / Smem::LW, tx = idx % Smem::LW;
			const int gx = x0 - R + tx, gy = y - R + ty;
			const bool in = gx >= 0 && gy >= 0 && gx < W && gy < H;
			S.lt[ty][tx] = in ? L.gray_tv[(size_t)gy*W + gx] : __builtin_nan("");
			S.sl[ty][tx] = in ? csL[(size_t)gy*W + gx] : 0;
		}
		for (int idx = tid; idx < CR_WT*SRH_ROWS_NR; idx += CR_THREADS) {
			const int pi = idx / SRH_ROWS_NR;
			const size_t qq = qbase + pi;
			S.rowinfo[pi][idx % SRH_ROWS_NR] = (x0 + pi < W) ? rowinfo[((qq >> 6)*SRH_ROWS_NR + idx % SRH_ROWS_NR)*64 + (qq & 63)] : 0u;
		}
		if (tid < CR_WT) S.meta[tid] = (x0 + tid < W) ? meta[qbase + tid] : 0;
	}
	__syncthreads();

	// ---- settle the reference side (one lane per pixel): a skipped tap's weight becomes +0.0; totalWeight and numPixels of
	// a fully usable other side -- the same additions in the same order (a skipped tap adds +0.0)
	if (g == 0) {
		double tw = 0.0;
		int np = 0;
		for (int row = 0; row < WS; ++row) {
			unsigned bits = 0;
			for (int col = 0; col < WS; ++col) {
				const double gl = S.lt[row][i + col], wt = S.w[row][i][col];
				const bool okl = gl == gl && wt > P.weight_cutoff;
				const double we = okl ? wt : 0.0;
				S.w[row][i][col] = we;
				tw += we;
				np += okl ? 1 : 0;
				bits |= (okl ? 1u : 0u) << col;
			}
			S.okl[row][i] = (unsigned short)bits;
		}
		S.totalW[i] = tw; S.npix[i] = np;
		const int nr = (x < W) ? S.meta[i] >> 16 : 0;
		int nblk = 0;
		for (int r = 0; r < nr; ++r) {
			S.blk0[i][r] = (unsigned short)nblk;
			nblk += ((int)(S.rowinfo[i][r] >> 16) + CR_NCB - 1)/CR_NCB;
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
		for (int task = g; task < ntask; task += CR_G) {
			while (task >= (int)S.blk0[i][r + 1]) ++r;
			const uint32_t info = S.rowinfo[i][r];
			const int xlo = (int)(short)(info & 0xffff), wdt = (int)(info >> 16);
			const int b = task - (int)S.blk0[i][r];
			const int cy = ymin + r;
			const int c0 = xlo + b*CR_NCB;
			const int nv = wdt - b*CR_NCB < CR_NCB ? wdt - b*CR_NCB : CR_NCB;
			n_dev += nv;
			double *const dst = crow + (size_t)task*CR_NCB*CR_WT;
			// (a span's candidates lie inside the other image; so do their windows when `full` says so)
			bool fast = true;
			for (int j = 0; j < nv; ++j) fast = fast && full_oth[(size_t)cy*OW + c0 + j] != 0;
			if (fast) {
				// the columns right of a partial block's last candidate are read clamped and their sums dropped
				double acc[CR_NCB];
#pragma unroll
				for (int j = 0; j < CR_NCB; ++j) acc[j] = 0.0;
#pragma unroll 1
				for (int row = 0; row < WS; ++row) {
					const uint64_t *rp = csR + (size_t)(cy - R + row)*OW;
					uint64_t rr[NR_];
#pragma unroll
					for (int k = 0; k < NR_; ++k) {
						int gx = c0 - R + k;
						gx = gx < OW ? gx : OW - 1;
						rr[k] = rp[gx];
					}
#pragma unroll
					for (int col = 0; col < WS; ++col) {
						const double we = S.w[row][i][col];
						const uint64_t sg = S.sl[row][i + col];
#pragma unroll
						for (int j = 0; j < CR_NCB; ++j) acc[j] = __builtin_fma(we, census_term(sg, rr[col + j]), acc[j]);
					}
				}
#pragma unroll
				for (int j = 0; j < CR_NCB; ++j)
					if (j < nv) dst[j*CR_WT] = bad_full ? P.bad_ret : acc[j] / tw_full;
			} else {
				double s[CR_NCB], t[CR_NCB];
				int np[CR_NCB];
#pragma unroll
				for (int j = 0; j < CR_NCB; ++j) { s[j] = 0.0; t[j] = 0.0; np[j] = 0; }
#pragma unroll 1
				for (int row = 0; row < WS; ++row) {
					const int gy = cy - R + row;
					const bool rowok = gy >= 0 && gy < OH;
					const size_t rbase = (size_t)(rowok ? gy : 0)*OW;
					const unsigned okbits = S.okl[row][i];
					uint64_t rr[NR_];
					bool rv[NR_];
#pragma unroll
					for (int k = 0; k < NR_; ++k) {
						const int gx = c0 - R + k;
						const bool in = rowok && gx >= 0 && gx < OW;
						const size_t at = rbase + (in ? gx : 0);
						rv[k] = in && Rv.mask[at] == 1;
						rr[k] = rv[k] ? csR[at] : 0;
					}
#pragma unroll
					for (int col = 0; col < WS; ++col) {
						const double wt = S.w[row][i][col];                 // (+0.0 where the reference side skips the tap)
						const uint64_t sg = S.sl[row][i + col];
						const bool okl = (okbits >> col) & 1u;
#pragma unroll
						for (int j = 0; j < CR_NCB; ++j) {
							const bool ok = okl && rv[col + j];
							const double we = ok ? wt : 0.0;
							s[j] = __builtin_fma(we, census_term(sg, rr[col + j]), s[j]);
							t[j] += we;
							np[j] += ok ? 1 : 0;
						}
					}
				}
#pragma unroll
				for (int j = 0; j < CR_NCB; ++j)
					if (j < nv) dst[j*CR_WT] = (np[j] <= 4 || t[j] <= 1e-10) ? P.bad_ret : s[j] / t[j];
			}
		}
	}
	block_count_add(&cnt->n_eval_device, n_dev);
}

bool launch_twoview_rows_census(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                int y0, int nrows, const double *wbuf, const uint8_t *full_oth,
                                const uint32_t *rowinfo, const int32_t *meta, double *cost, int smax, Counters *cnt)
{
	const size_t items = (size_t)((width + SRH_WTILE - 1)/SRH_WTILE)*(SRH_WTILE/CR_WT)*nrows;
	const dim3 grid((unsigned)items);
#define SRH_RC(RR) case RR: hipLaunchKernelGGL(twoview_rows_census_kernel<RR>, grid, dim3(CR_THREADS), 0, st, views, ref, oth, P, \
	                                           y0, nrows, wbuf, full_oth, rowinfo, meta, cost, smax, cnt); return true;
	switch (P.window_radius) { SRH_RC(1) SRH_RC(2) SRH_RC(3) SRH_RC(4) SRH_RC(5) default: return false; }
#undef SRH_RC
}

// ------------------------------------------------------------------ list-order costs
// steep curves (list_mode 2): one wave per reference pixel, a lane per list entry, tv_cost_census on the tile-major window
__global__ __launch_bounds__(64)
void twoview_list_census_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P,
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
			cost[q*(size_t)cmax + k] = tv_cost_census(L, Rv, wq, SRH_WTILE, P, x, y, (int)(e & 0xffffu), (int)(e >> 16));
			++n_dev;
		}
	}
	block_count_add(&cnt->n_eval_device, n_dev);
}

void launch_twoview_list_census(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                int y0, int nrows, const double *wbuf, const int32_t *count, const uint32_t *cand,
                                double *cost, int cmax, Counters *cnt)
{
	const size_t n = (size_t)nrows*width;
	hipLaunchKernelGGL(twoview_list_census_kernel, dim3((unsigned)n), dim3(64), 0, st,
	                   views, ref, oth, P, y0, nrows, wbuf, count, cand, cost, cmax, cnt);
}

} // namespace srh
