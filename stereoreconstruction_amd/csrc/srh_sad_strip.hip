// srh_sad_strip.hip -- TwoViewStereo::cost_sad (stereo/twoviewstereo.cpp:864-905) for row-aligned rigs as a PERSISTENT
// kernel that fills the dense plan's cost rows (option "sad_dense"): the frame of
// twoview_strip_cost_kernel's 4-wave form (srh_stripframe.hpp: shared, not copied), the sums of twoview_rows_sad_kernel
// (srh_sad.hip).
//
//   * a workgroup owns a vertical strip of one tile column (work items from the ticket counter, tall items first) and
//     keeps the rows of both views in an LDS ring of 2R+2 slots: one new row per view and tile;
//   * every input enters LDS by LDS-DMA: the windows (layout B, as the weights kernels write them), the pixels' candidate
//     ranges (pixel_range_kernel), the "window fully usable" bytes of the other view, and the image rows from NaN-bordered
//     planes -- the reference side from gray_tv (sample() behind the left mask), the other side from the masked gray plane
//     (pixel() behind the right mask: usable on the last column and row too), so no lane ever tests a bound;
//   * the next tile's row and ranges are requested under the current tile's arithmetic.
//
// cost_sad has one sweep over the window.  What the reference pixel's own side skips is settled once per tile: a skipped
// tap's weight becomes +0.0 in the LDS window and its gray value 0.0, a bit per tap remembers which ones count.  A
// candidate whose window in the other view is fully usable then costs, per tap, a subtraction (the absolute value a
// source modifier), a minimum, a multiply and an add -- never fused -- and its totalWeight and numPixels are the pixel's
// (fast form).  Any other candidate takes the select form: every tap guarded, a skipped tap adds +0.0, numPixels and
// totalWeight per candidate.  Every column of [lo, hi] of every pixel is written: no fill kernel runs behind this one.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"

#include <type_traits>

namespace srh {

#define SS_G 8                        // block lanes per pixel
#define SS_NT 256                      // threads: 4 waves, 8 pixels x 8 block lanes each

// ------------------------------------------------------------------ padded planes (padded_raster_kernel, srh_stripframe.hpp)
// gray(x, y) where the mask is WHITE, NaN elsewhere and outside the image: cost_sad's other-side tap (right.pixel()
// behind rightMask; sad_tap, srh_walk.hpp)
struct PaddedGray {
	const double *gray; const uint8_t *mask; int W;
	__device__ double operator()(int x, int y, bool in) const {
		return (in && mask[(size_t)y*W + x] == 1) ? gray[(size_t)y*W + x] : __builtin_nan("");
	}
};
void launch_padded_gray(hipStream_t st, const double *gray, const uint8_t *mask, int w, int h, double *out) {
	launch_padded_raster(st, w, h, out, PaddedGray{ gray, mask, w });
}

// zero-bordered copy of a W x H byte plane (sad_full_window_kernel's)
struct PaddedBytes {
	const uint8_t *in; int W;
	__device__ uint8_t operator()(int x, int y, bool inside) const { return inside ? in[(size_t)y*W + x] : 0; }
};
void launch_padded_bytes(hipStream_t st, const uint8_t *in, int w, int h, uint8_t *out) {
	launch_padded_raster(st, w, h, out, PaddedBytes{ in, w });
}

// ------------------------------------------------------------------ the kernel
struct SadStripArgs {
	int W, H, y0, nrows;                    // reference view size; rows [y0, y0 + nrows) of it
	const double *wimg;                     // windows of the band, layout B
	const PixRange *prange;                 // candidate column range per pixel of the band
	const double *ref_tvp;                  // NaN-bordered gray_tv plane of the reference view
	const double *oth_grayp;                // NaN-bordered masked gray plane of the other view
	const uint8_t *oth_fullp;               // zero-bordered cost_sad "window fully usable" plane of the other view
	double *cost; int cstride;              // cost rows, tile-transposed: ((tile*cstride) + k)*32 + pixel
	Counters *cnt;
	StripItems items;                       // the band's work items (srh_stripframe.hpp)
	double weight_cutoff, bad_ret, max_color_diff;
};

template <int R>
struct SadStripSmem : StripGeom<R> {
	typedef StripGeom<R> G;                    // the tile and staging geometry (srh_stripframe.hpp)
	alignas(16) double w[G::WS][STRIP_TP][G::WP];    // LDS image of the windows: [row][pixel][tap]; per tile, a skipped tap's weight -> +0.0
	alignas(16) double rt[G::NS][G::RW];       // ring: the other view's rows (NaN: tap unusable)
	alignas(16) double lt[G::NS][G::LW];       // ring: the reference rows (NaN: tap unusable)
	alignas(16) double l0[G::WS][G::LW];       // the current window's reference rows, NaN -> 0.0 (by window row, not ring slot)
	alignas(16) PixRange pr[2][STRIP_TP];
	alignas(16) unsigned char full[2][G::FW];
	unsigned short okm[G::WS][STRIP_TP];       // bit col: tap (row, col) of the pixel counts on the reference side
	unsigned short glist[STRIP_TP*G::NBMAX];   // select-form work list: pixel*64 + block
	int glist_n;
	int item;
	static_assert(G::NBMAX <= 64, "work-list entry = pixel*64 + block");
};

static_assert(sizeof(SadStripSmem<5>) <= 80*1024 && sizeof(SadStripSmem<2>) <= 80*1024, "two workgroups share a CU's 160 KB of LDS");

// One 8-column block of pixel `pi` in the select form (the select form of twoview_rows_sad_kernel, the rows taken from
// the rings): every tap guarded, a skipped tap adds +0.0, numPixels and totalWeight per candidate.  Candidates whose bit
// is set in `store` are written.  (S.w holds the weight itself wherever the reference side counts.)
template <int R>
__device__ __forceinline__ void sad_strip_select_block(const SadStripSmem<R> &S, int s0, int pi, int rc, unsigned store,
                                                    double *__restrict__ dst, double bad_ret, double mcd)
{
	typedef SadStripSmem<R> Smem;
	constexpr int WS = Smem::WS, NS = Smem::NS, NCB = STRIP_NCB, NR = NCB + 2*R;
	double s[NCB], t[NCB];
	int np[NCB];
#pragma unroll
	for (int j = 0; j < NCB; ++j) { s[j] = 0.0; t[j] = 0.0; np[j] = 0; }
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const unsigned okm = S.okm[row][pi];
		if (okm == 0) continue;                                // (no tap of this window row counts: every term a skipped +0.0)
		const int sl = ring_slot(s0, row, NS);
		double rr[NR];
		bool rv[NR];
		const double2 *rp = reinterpret_cast<const double2 *>(&S.rt[sl][rc]);
#pragma unroll
		for (int m = 0; m < NR/2; ++m) { const double2 v = rp[m]; rr[2*m] = v.x; rr[2*m + 1] = v.y; }
#pragma unroll
		for (int m = 0; m < NR; ++m) { rv[m] = rr[m] == rr[m]; rr[m] = rv[m] ? rr[m] : 0.0; }
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const double gl = S.l0[row][pi + col], wt = S.w[row][pi][col];
			const bool okl = (okm >> col) & 1u;
#pragma unroll
			for (int j = 0; j < NCB; ++j) {
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
	for (int j = 0; j < NCB; ++j)
		if ((store >> j) & 1u) dst[(ptrdiff_t)j*STRIP_TP] = (np[j] <= 4 || t[j] <= 1e-10) ? bad_ret : s[j] / t[j];
}

template <int R>
__global__ __launch_bounds__(SS_NT, 2)
void twoview_strip_sad_kernel(const SadStripArgs A)
{
	typedef SadStripSmem<R> Smem;
	constexpr int WS = Smem::WS, WP = Smem::WP, WPIX = Smem::WPIX, LW = Smem::LW, NS = Smem::NS;
	constexpr int NCB = STRIP_NCB, CHUNK = STRIP_CHUNK, G = SS_G, NT = SS_NT;
	constexpr int NR = NCB + 2*R;              // right-row values a block needs (even)
	static_assert(NR % 2 == 0, "16-byte rows");
	extern __shared__ __align__(16) unsigned char smem_raw[];
	Smem &S = *reinterpret_cast<Smem *>(smem_raw);
	const Smem &CS = S;

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int i = wv*8 + (lane & 7);             // pixel within the tile: the wave owns pixels 8*wv .. 8*wv + 7
	const int g = lane >> 3;                     // block lane of the pixel
	const int W = A.W;
	const int tiles_per_row = (W + STRIP_TP - 1)/STRIP_TP;
	const int SP = padded_stride(W);
	const double mcd = A.max_color_diff;
	const bool fast_ok = mcd == mcd;             // (fmin and the reference's select agree for any non-NaN bound; srh_sad.hip)
	unsigned n_dev = 0;

	for (;;) {
		// ---- next work item: (row segment, tile column); tall segments first, so the tail of the launch is short
		const int item = strip_draw_item(&A.cnt->strip_ticket, &S.item, tid);
		if (item >= A.items.nitems) break;
		int tx, ya, nh;
		A.items.segment(item, tiles_per_row, A.nrows, tx, ya, nh);
		const int x0 = tx*STRIP_TP;
		const int x = x0 + i;
		int cs = 0, rowbase = 0;                   // staging origin (column, even) and the image row held by slot 0

		// one tile's own inputs (nothing here depends on the staging origin): ranges, windows
		auto issue_tile_inputs = [&](int r, int buf, bool ranges, bool windows) {
			const size_t px0 = (size_t)r*W + x0;
			if (ranges && wv == 1) strip_dma4(A.prange + px0, &S.pr[buf][0], STRIP_TP*8, lane);
			if (windows) {
				// each wave its own pixels' windows (8 pixels x WP taps of every window row): nobody else touches them
				// outside the select form
				const double *wt = A.wimg + ((size_t)r*tiles_per_row + tx)*(size_t)(STRIP_TP*WPIX);
				for (int a = 0; a < WS; ++a)
					strip_dma16(wt + (size_t)a*(STRIP_TP*WP) + wv*8*WP, &S.w[a][wv*8][0], 8*WP*8, lane);
			}
		};
		// image row `yy` of both views into ring slot `sl`; "full" bytes of row `fy` into full[fb] (the last wave)
		auto issue_row = [&](int yy, int sl) {
			strip_request_row<R>(A.oth_grayp, A.ref_tvp, SP, yy, cs, x0, &S.rt[sl][0], &S.lt[sl][0], wv, lane);
		};
		auto issue_full = [&](int fy, int fb) {
			if (wv == 3) strip_request_full<R>(A.oth_fullp, SP, fy, cs, &S.full[fb][0], lane);
		};

		bool first = true;
		for (int r = ya; r < ya + nh; ++r) {
			const int y = A.y0 + r;
			const int cur = (r - ya) & 1, nxt = cur ^ 1;
			const bool has_next = r + 1 < ya + nh;
			if (first) issue_tile_inputs(r, cur, true, true);
			// ---- A: everything requested for this tile has landed and every wave has left the previous tile
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__builtin_amdgcn_s_barrier();

			// ---- B: the tile's candidate ranges (every wave works out the union for itself: 32 values)
			int cmax, cmin_raw;
			{
				const int pi = lane & 31;
				int lo, hi;
				strip_pixel_range(CS.pr[cur][pi], x0 + pi < W, lo, hi);
				tile_range_union(lo, hi, cmin_raw, cmax);
			}
			const int cmin = cmin_raw & ~1;
			const bool any = cmin_raw <= cmax;
			if (needs_restage(first, any, cmin, cmax, cs)) {
				if (!first) __builtin_amdgcn_s_barrier();          // (a restage in mid-strip: nobody reads the rings any more)
				cs = any ? cmin : 0;
				rowbase = y - R;
				for (int rr = 0; rr < WS; ++rr) issue_row(y - R + rr, rr);
				issue_full(y, cur);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__builtin_amdgcn_s_barrier();
			}
			strip_clamp_to_chunk(any, cs, cmax, tid, &A.cnt->strip_overflow);
			first = false;
			const int s0 = (y - R - rowbase) % NS;                   // ring slot of the window's first row

			// ---- the reference side of the tile, once: which taps count (sample() valid, weight above the cut-off); a
			// skipped tap's weight becomes +0.0 and its gray value 0.0, so that it adds 0 * min(|0 - r|, MAX) = +0.0 in
			// the fast form; a bit per tap for the select form.  Each wave its own pixels' windows.
			for (int row = g; row < WS; row += G) {
				const int sl = ring_slot(s0, row, NS);
				unsigned m = 0;
#pragma unroll
				for (int col = 0; col < WS; ++col) {
					const double gl = CS.lt[sl][i + col], wt = CS.w[row][i][col];
					const bool okl = gl == gl && wt > A.weight_cutoff;
					S.w[row][i][col] = okl ? wt : 0.0;
					m |= okl ? 1u << col : 0u;
				}
				S.okm[row][i] = (unsigned short)m;
			}
			for (int k = tid; k < WS*LW; k += NT) {
				const int row = k / LW, cc = k - row*LW;
				const int sl = ring_slot(s0, row, NS);
				const double v = CS.lt[sl][cc];
				S.l0[row][cc] = v == v ? v : 0.0;
			}
			__syncthreads();                                       // (no LDS-DMA in flight here: a bare barrier)

			// ---- request the next tile's row and ranges now: they travel under the block loops
			if (has_next) {
				issue_row(y + R + 1, (y + R + 1 - rowbase) % NS);
				issue_full(y + 1, nxt);
				issue_tile_inputs(r + 1, nxt, true, false);
			}
			const unsigned char *rfull = &CS.full[cur][full_offset(y, SP, cs)];

			// ---- does any candidate of the tile need the select form?  (uniform: every wave looks at the whole tile)
			bool need_select = false;
			{
				bool bad = false;
#pragma unroll
				for (int it = 0; it < (CHUNK + 63)/64; ++it) {
					const int k = it*64 + lane, c = cs + k;
					if (k < CHUNK && c >= cmin_raw && c <= cmax && rfull[k] == 0) bad = true;
				}
				need_select = (any && !fast_ok) || __any(bad) != 0;
			}

			// ---- this lane's pixel
			int e_min, e_max;
			{
				strip_pixel_range(CS.pr[cur][i], x < W, e_min, e_max);
				if (e_max > e_min + A.cstride - 1) e_max = e_min + A.cstride - 1;   // (pixel_range_kernel never leaves more)
			}
			const size_t tile = (size_t)r*tiles_per_row + tx;
			if (e_max >= e_min) {
				// the pixel's totalWeight and numPixels when the other side is fully usable: the reference's additions in its
				// order (a skipped tap adds +0.0), on every block lane of the pixel alike
				double tw = 0.0;
				int npx = 0;
#pragma unroll 1
				for (int row = 0; row < WS; ++row) {
#pragma unroll
					for (int col = 0; col < WS; ++col) tw += CS.w[row][i][col];
					npx += __builtin_popcount((unsigned)CS.okm[row][i]);
				}
				const bool bad_full = npx <= 4 || tw <= 1e-10;
				int lo, hi, lo_e, nblocks;
				strip_lane_blocks<true>(e_min, e_max, cs, lo, hi, lo_e, nblocks);   // blocks start on even columns (>= cs)
				double *crow = A.cost + tile*(size_t)A.cstride*STRIP_TP + i;
				// phase 1: blocks of NCB candidates in the fast form
				for (int b = g; b < (fast_ok ? nblocks : 0); b += G) {
					const int c0 = lo_e + b*NCB;
					const int rc = c0 - cs;                 // tile column of the window's left edge (even)
					// bit j: candidate c0 + j is inside the pixel's range and its window in the other view is fully usable
					unsigned vm = 0;
#pragma unroll
					for (int j = 0; j < NCB; ++j) {
						const int c = c0 + j;
						vm |= (c >= lo && c <= hi && rfull[rc + j] != 0) ? 1u << j : 0u;
					}
					if (vm == 0) continue;
					n_dev += __builtin_popcount(vm);
					// one sweep over the window for the first NC candidates of the block
					auto sweep = [&](auto nc_c) {
						constexpr int NC = decltype(nc_c)::value, NRC = NC + 2*R;
						double acc[NC];
#pragma unroll
						for (int j = 0; j < NC; ++j) acc[j] = 0.0;
#pragma unroll 1
						for (int row = 0; row < WS; ++row) {
							const int sl = ring_slot(s0, row, NS);
							double rr[NRC], we[WP], gl[WS];
							const double2 *rp = reinterpret_cast<const double2 *>(&CS.rt[sl][rc]);
							const double2 *wp = reinterpret_cast<const double2 *>(&CS.w[row][i][0]);
#pragma unroll
							for (int m = 0; m < NRC/2; ++m) { const double2 v = rp[m]; rr[2*m] = v.x; rr[2*m + 1] = v.y; }
#pragma unroll
							for (int m = 0; m < WP/2; ++m) { const double2 v = wp[m]; we[2*m] = v.x; we[2*m + 1] = v.y; }
#pragma unroll
							for (int col = 0; col < WS; ++col) gl[col] = CS.l0[row][i + col];
#pragma unroll
							for (int col = 0; col < WS; ++col) {
#pragma unroll
								for (int j = 0; j < NC; ++j) acc[j] += we[col]*__builtin_fmin(fabs(gl[col] - rr[col + j]), mcd);
							}
						}
#pragma unroll
						for (int j = 0; j < NC; ++j)
							if ((vm >> j) & 1u) crow[(size_t)(c0 + j - e_min)*STRIP_TP] = bad_full ? A.bad_ret : acc[j] / tw;
					};
					// a pixel's last block often holds one or two columns only (the alignment pad in front, a range of 8k + 1
					// columns) and is a round of the block lanes all by itself: it is swept two candidates wide
					if (hi - c0 < 2) sweep(std::integral_constant<int, 2>());
					else sweep(std::integral_constant<int, NCB>());
				}
			}
			// phase 2: the remaining candidates in the select form (image borders, masked taps of the other view), 8-column
			// blocks compacted into an LDS work list and spread over all lanes of the workgroup
			if (need_select) {
				if (tid == 0) S.glist_n = 0;
				__syncthreads();
				auto block_need = [&](int pi, int b, int &c0, int &qlo) -> unsigned {
					int qhi;
					strip_pixel_range(CS.pr[cur][pi], x0 + pi < W, qlo, qhi);
					if (qhi > qlo + A.cstride - 1) qhi = qlo + A.cstride - 1;
					if (qhi > cs + CHUNK - 1) qhi = cs + CHUNK - 1;
					const int ql = qlo > cs ? qlo : cs;
					c0 = (ql & ~1) + b*NCB;
					if (qhi < ql || c0 > qhi) return 0u;
					unsigned need = 0;
#pragma unroll
					for (int j = 0; j < NCB; ++j) {
						const int c = c0 + j;
						if (c >= ql && c <= qhi && (!fast_ok || rfull[c - cs] == 0)) need |= 1u << j;
					}
					return need;
				};
				for (int p = tid; p < STRIP_TP*Smem::NBMAX; p += NT) {
					const int pi = p / Smem::NBMAX, b = p - pi*Smem::NBMAX;
					int c0, qlo;
					if (block_need(pi, b, c0, qlo)) S.glist[atomicAdd(&S.glist_n, 1)] = (unsigned short)(pi*64 + b);
				}
				__syncthreads();
				const int nblk = CS.glist_n;
				for (int q = tid; q < nblk; q += NT) {
					const int pi = CS.glist[q] >> 6, b = CS.glist[q] & 63;
					int c0, qlo;
					const unsigned store = block_need(pi, b, c0, qlo);
					n_dev += __builtin_popcount(store);
					sad_strip_select_block<R>(CS, s0, pi, c0 - cs, store,
					                          A.cost + (tile*(size_t)A.cstride)*STRIP_TP + (ptrdiff_t)(c0 - qlo)*STRIP_TP + pi,
					                          A.bad_ret, mcd);
				}
				__syncthreads();     // the select form reads any pixel's window: all of it done before a window is replaced
			}
			// ---- the wave replaces its own pixels' windows as soon as it has left them
			if (has_next) issue_tile_inputs(r + 1, nxt, false, true);
		}
	}
	block_count_add(&A.cnt->n_eval_device, n_dev);
}

bool launch_twoview_strip_sad(hipStream_t st, int width, int height, const srh_params &P, int y0, int nrows,
                              const double *wimg, const PixRange *prange, const double *ref_tvp, const double *oth_grayp,
                              const uint8_t *oth_fullp, double *cost, int cstride, Counters *cnt, int num_cus)
{
	SadStripArgs a;
	a.W = width; a.H = height; a.y0 = y0; a.nrows = nrows;
	a.wimg = wimg; a.prange = prange;
	a.ref_tvp = ref_tvp; a.oth_grayp = oth_grayp; a.oth_fullp = oth_fullp;
	a.cost = cost; a.cstride = cstride; a.cnt = cnt;
	a.weight_cutoff = P.weight_cutoff; a.bad_ret = P.bad_ret; a.max_color_diff = P.max_color_diff;
	a.items = StripItems::cut(nrows, width);
	// two workgroups per compute unit
	switch (P.window_radius) {
	case 5: launch_strip(st, twoview_strip_sad_kernel<5>, a, sizeof(SadStripSmem<5>), SS_NT, 2, num_cus, a.items.nitems); return true;
	case 2: launch_strip(st, twoview_strip_sad_kernel<2>, a, sizeof(SadStripSmem<2>), SS_NT, 2, num_cus, a.items.nitems); return true;
	default: return false;
	}
}

} // namespace srh
