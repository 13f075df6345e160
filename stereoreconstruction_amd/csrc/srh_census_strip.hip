// srh_census_strip.hip -- the support-weighted census cost (option "cost" = SRH_COST_CENSUS) for row-aligned
// rigs as a PERSISTENT kernel that fills the dense plan's cost rows (option "census_dense"): the frame of
// twoview_strip_sad_kernel (srh_stripframe.hpp: shared, not copied), the sums of twoview_rows_census_kernel (srh_census.hip)
// as srh_census_block.hpp states them.
//
//   * a workgroup owns a vertical strip of one tile column (work items from the ticket counter, tall items first) and
//     keeps the signature rows of both views in an LDS ring of 2R+2 slots: one new row per view and tile;
//   * every input enters LDS by LDS-DMA: the windows (layout B), the pixels' candidate ranges, the "window fully usable"
//     bytes of the other view (cost_sad's plane: the same definition) and the signature rows from planes in the padded
//     raster, 8 bytes per pixel, whose unusable taps -- outside the image, behind the mask; on the reference side wherever
//     gray_tv is NaN -- hold CENSUS_UNUSABLE, so no lane ever tests a bound;
//   * the next tile's row and ranges are requested under the current tile's arithmetic.
//
// What the reference pixel's own side skips is settled once per tile: a skipped tap's weight becomes +0.0 in the LDS
// window, a bit per tap remembers which ones count.  A candidate whose window in the other view is fully usable then costs,
// per tap, two XORs, two population counts, a convert and one fused multiply-add, and its totalWeight and numPixels are
// the pixel's (fast form).  Any other candidate takes the select form: every tap guarded, numPixels and totalWeight per
// candidate.  Every column of [lo, hi] of every pixel is written: no fill kernel runs behind this one.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_census_block.hpp"

#include <type_traits>

namespace srh {

#define CSK_G 8                        // block lanes per pixel
#define CSK_NT 256                     // threads: 4 waves, 8 pixels x 8 block lanes each

// ------------------------------------------------------------------ padded planes (padded_raster_kernel, srh_stripframe.hpp)
// the other side's tap: the signature where the pixel is inside and its mask is WHITE (tv_cost_census's okr)
struct PaddedCensusOther {
	const uint64_t *census; const uint8_t *mask; int W;
	__device__ uint64_t operator()(int x, int y, bool in) const {
		return (in && mask[(size_t)y*W + x] == 1) ? census[(size_t)y*W + x] : CENSUS_UNUSABLE;
	}
};
// the reference side's tap: the signature where gray_tv is not NaN (cost_sad's left-tap rule, tv_tap)
struct PaddedCensusRef {
	const uint64_t *census; const double *gray_tv; int W;
	__device__ uint64_t operator()(int x, int y, bool in) const {
		if (!in) return CENSUS_UNUSABLE;
		const double g = gray_tv[(size_t)y*W + x];
		return g == g ? census[(size_t)y*W + x] : CENSUS_UNUSABLE;
	}
};
void launch_padded_census(hipStream_t st, const uint64_t *census, const uint8_t *mask, const double *gray_tv, int w, int h,
                          uint64_t *out_other, uint64_t *out_ref) {
	launch_padded_raster(st, w, h, out_other, PaddedCensusOther{ census, mask, w });
	launch_padded_raster(st, w, h, out_ref, PaddedCensusRef{ census, gray_tv, w });
}

// ------------------------------------------------------------------ the kernel
struct CensusStripArgs {
	int W, H, y0, nrows;                    // reference view size; rows [y0, y0 + nrows) of it
	const double *wimg;                     // windows of the band, layout B
	const PixRange *prange;                 // candidate column range per pixel of the band
	const uint64_t *ref_cenp;               // the reference view's signatures, reference side (PaddedCensusRef)
	const uint64_t *oth_cenp;               // the other view's signatures, other side (PaddedCensusOther)
	const uint8_t *oth_fullp;               // zero-bordered cost_sad "window fully usable" plane of the other view
	double *cost; int cstride;              // cost rows, tile-transposed: ((tile*cstride) + k)*32 + pixel
	Counters *cnt;
	StripItems items;                       // the band's work items (srh_stripframe.hpp)
	double weight_cutoff, bad_ret;
};

template <int R>
struct CensusStripSmem : StripGeom<R> {
	typedef StripGeom<R> G;                    // the tile and staging geometry (srh_stripframe.hpp)
	alignas(16) double w[G::WS][STRIP_TP][G::WP];    // LDS image of the windows: [row][pixel][tap]; per tile, a skipped tap's weight -> +0.0
	alignas(16) uint64_t rt[G::NS][G::RW];     // ring: the other view's signature rows (CENSUS_UNUSABLE: tap unusable)
	alignas(16) uint64_t lt[G::NS][G::LW];     // ring: the reference view's signature rows
	alignas(16) PixRange pr[2][STRIP_TP];
	alignas(16) unsigned char full[2][G::FW];
	unsigned short okm[G::WS][STRIP_TP];       // bit col: tap (row, col) of the pixel counts on the reference side
	unsigned short glist[STRIP_TP*G::NBMAX];   // select-form work list: pixel*64 + block
	int glist_n;
	int item;
	static_assert(G::NBMAX <= 64, "work-list entry = pixel*64 + block");
};

static_assert(sizeof(CensusStripSmem<5>) <= 80*1024 && sizeof(CensusStripSmem<2>) <= 80*1024, "two workgroups share a CU's 160 KB of LDS");

// the row source of srh_census_block.hpp: the window of tile pixel `pi` against the block whose first candidate's left tap
// is staged column `rc`, the rows taken from the rings (the window's first row in slot s0)
template <int R>
struct CensusStripRows {
	const CensusStripSmem<R> *S; int s0, pi, rc;
	__device__ __forceinline__ CensusRow row(int row) const {
		const int sl = ring_slot(s0, row, CensusStripSmem<R>::NS);
		return CensusRow{ &S->rt[sl][rc], &S->w[row][pi][0], &S->lt[sl][pi], S->okm[row][pi] };
	}
};

template <int R>
__global__ __launch_bounds__(CSK_NT, 2)
void twoview_strip_census_kernel(const CensusStripArgs A)
{
	typedef CensusStripSmem<R> Smem;
	constexpr int WS = Smem::WS, WP = Smem::WP, WPIX = Smem::WPIX, NS = Smem::NS;
	constexpr int NCB = STRIP_NCB, CHUNK = STRIP_CHUNK, G = CSK_G, NT = CSK_NT;
	static_assert((NCB + 2*R) % 2 == 0, "16-byte rows");
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
			strip_request_row<R>(A.oth_cenp, A.ref_cenp, SP, yy, cs, x0, &S.rt[sl][0], &S.lt[sl][0], wv, lane);
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

			// ---- the reference side of the tile, once (census_settle_row).  Each wave its own pixels' windows.
			for (int row = g; row < WS; row += G)
				S.okm[row][i] = (unsigned short)census_settle_row<WS>(&CS.lt[ring_slot(s0, row, NS)][i], &S.w[row][i][0], A.weight_cutoff);
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
				need_select = __any(bad) != 0;
			}

			// ---- this lane's pixel
			int e_min, e_max;
			{
				strip_pixel_range(CS.pr[cur][i], x < W, e_min, e_max);
				if (e_max > e_min + A.cstride - 1) e_max = e_min + A.cstride - 1;   // (pixel_range_kernel never leaves more)
			}
			const size_t tile = (size_t)r*tiles_per_row + tx;
			if (e_max >= e_min) {
				// the pixel's totalWeight and numPixels when the other side is fully usable, on every block lane of the pixel alike
				double tw;
				int npx;
				census_pixel_totals<WS>(CensusStripRows<R>{ &CS, s0, i, 0 }, tw, npx);
				int lo, hi, lo_e, nblocks;
				strip_lane_blocks<true>(e_min, e_max, cs, lo, hi, lo_e, nblocks);   // blocks start on even columns (>= cs)
				double *crow = A.cost + tile*(size_t)A.cstride*STRIP_TP + i;
				// phase 1: blocks of NCB candidates in the fast form
				for (int b = g; b < nblocks; b += G) {
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
						constexpr int NC = decltype(nc_c)::value;
						double acc[NC];
						census_fast_block<WS, NC>(CensusStripRows<R>{ &CS, s0, i, rc }, acc);
#pragma unroll
						for (int j = 0; j < NC; ++j)
							if ((vm >> j) & 1u) crow[(size_t)(c0 + j - e_min)*STRIP_TP] = census_finish(npx, tw, acc[j], A.bad_ret);
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
						if (c >= ql && c <= qhi && rfull[c - cs] == 0) need |= 1u << j;
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
					double s[NCB], t[NCB];
					int np[NCB];
					census_select_block<WS, NCB>(CensusStripRows<R>{ &CS, s0, pi, c0 - cs }, s, t, np);
					double *dst = A.cost + (tile*(size_t)A.cstride)*STRIP_TP + (ptrdiff_t)(c0 - qlo)*STRIP_TP + pi;
#pragma unroll
					for (int j = 0; j < NCB; ++j)
						if ((store >> j) & 1u) dst[(ptrdiff_t)j*STRIP_TP] = census_finish(np[j], t[j], s[j], A.bad_ret);
				}
				__syncthreads();     // the select form reads any pixel's window: all of it done before a window is replaced
			}
			// ---- the wave replaces its own pixels' windows as soon as it has left them
			if (has_next) issue_tile_inputs(r + 1, nxt, false, true);
		}
	}
	block_count_add(&A.cnt->n_eval_device, n_dev);
}

bool launch_twoview_strip_census(hipStream_t st, int width, int height, const srh_params &P, int y0, int nrows,
                                 const double *wimg, const PixRange *prange, const uint64_t *ref_cenp, const uint64_t *oth_cenp,
                                 const uint8_t *oth_fullp, double *cost, int cstride, Counters *cnt, int num_cus)
{
	CensusStripArgs a;
	a.W = width; a.H = height; a.y0 = y0; a.nrows = nrows;
	a.wimg = wimg; a.prange = prange;
	a.ref_cenp = ref_cenp; a.oth_cenp = oth_cenp; a.oth_fullp = oth_fullp;
	a.cost = cost; a.cstride = cstride; a.cnt = cnt;
	a.weight_cutoff = P.weight_cutoff; a.bad_ret = P.bad_ret;
	a.items = StripItems::cut(nrows, width);
	// two workgroups per compute unit
	switch (P.window_radius) {
	case 5: launch_strip(st, twoview_strip_census_kernel<5>, a, sizeof(CensusStripSmem<5>), CSK_NT, 2, num_cus, a.items.nitems); return true;
	case 2: launch_strip(st, twoview_strip_census_kernel<2>, a, sizeof(CensusStripSmem<2>), CSK_NT, 2, num_cus, a.items.nitems); return true;
	default: return false;
	}
}

} // namespace srh
