// srh_sad_strip.hip -- TwoViewStereo::cost_sad (stereo/twoviewstereo.cpp:864-905) for row-aligned rigs as a PERSISTENT
// kernel that fills the dense plan's cost rows (option "sad_dense"): the structure of
// twoview_strip_cost_kernel (srh_strip.hip, 4-wave form), the sums of twoview_rows_sad_kernel (srh_sad.hip).
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

#define SS_TP 32                       // pixels per tile (= SRH_WTILE)
#define SS_NCB 8                       // candidate columns per block
#define SS_G 8                         // block lanes per pixel
#define SS_NT 256                      // threads: 4 waves, 8 pixels x 8 block lanes each
#define SS_CHUNK 320                   // candidate columns a tile can hold in LDS (= strip_chunk_columns())

typedef __attribute__((address_space(3))) void ss_lds_void;
typedef __attribute__((address_space(1))) const void ss_gbl_void;

// ------------------------------------------------------------------ padded planes
// out[(y+PADY)*SP + x+PADL] = gray(x, y) where the mask is WHITE, NaN elsewhere and outside the image: cost_sad's
// other-side tap (right.pixel() behind rightMask; sad_tap, srh_walk.hpp)
__global__ void padded_gray_kernel(const double *__restrict__ gray, const uint8_t *__restrict__ mask, int W, int H,
                                   double *__restrict__ out)
{
	const int SP = padded_stride(W), HP = H + 2*SRH_PADY;
	const size_t n = (size_t)SP*HP;
	const double nan = __builtin_nan("");
	for (size_t k = (size_t)blockIdx.x*blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x*blockDim.x) {
		const int x = (int)(k % (size_t)SP) - SRH_PADL, y = (int)(k / (size_t)SP) - SRH_PADY;
		const bool in = x >= 0 && y >= 0 && x < W && y < H;
		out[k] = (in && mask[(size_t)y*W + x] == 1) ? gray[(size_t)y*W + x] : nan;
	}
}

void launch_padded_gray(hipStream_t st, const double *gray, const uint8_t *mask, int w, int h, double *out) {
	size_t n = padded_size(w, h);
	size_t b = (n + 255)/256; if (b > 4096) b = 4096;
	hipLaunchKernelGGL(padded_gray_kernel, dim3((unsigned)b), dim3(256), 0, st, gray, mask, w, h, out);
}

// zero-bordered copy of a W x H byte plane (sad_full_window_kernel's) on the padded raster
__global__ void padded_bytes_kernel(const uint8_t *__restrict__ in, int W, int H, uint8_t *__restrict__ out)
{
	const int SP = padded_stride(W), HP = H + 2*SRH_PADY;
	const size_t n = (size_t)SP*HP;
	for (size_t k = (size_t)blockIdx.x*blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x*blockDim.x) {
		const int x = (int)(k % (size_t)SP) - SRH_PADL, y = (int)(k / (size_t)SP) - SRH_PADY;
		out[k] = (x >= 0 && y >= 0 && x < W && y < H) ? in[(size_t)y*W + x] : 0;
	}
}

void launch_padded_bytes(hipStream_t st, const uint8_t *in, int w, int h, uint8_t *out) {
	size_t n = padded_size(w, h);
	size_t b = (n + 255)/256; if (b > 4096) b = 4096;
	hipLaunchKernelGGL(padded_bytes_kernel, dim3((unsigned)b), dim3(256), 0, st, in, w, h, out);
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
	int n1, n2;                             // rows [0,n1) in 16-row items, [n1,n2) in 8-row items, the rest in 4-row items
	int nitems;
	double weight_cutoff, bad_ret, max_color_diff;
};

// work items as the NCC strip kernel cuts them: 3/4 of the rows in 16-row items, 2/3 of the rest in 8-row items, the
// remainder in 4-row items
static void sad_strip_items(SadStripArgs &a) {
	a.n1 = ((a.nrows*3/4)/16)*16;
	a.n2 = a.n1 + (((a.nrows - a.n1)*2/3)/8)*8;
	const int nseg = a.n1/16 + (a.n2 - a.n1)/8 + (a.nrows - a.n2 + 3)/4;
	a.nitems = nseg*((a.W + SS_TP - 1)/SS_TP);
}

template <int R>
struct SadStripSmem {
	static constexpr int WS = 2*R + 1;
	static constexpr int WP = (WS + 1) & ~1;                 // taps per window row, padded even
	static constexpr int WPIX = WS*WP;                       // doubles per pixel window
	static constexpr int RW = SS_CHUNK + 2*R + SS_NCB + 2;   // staged width of the other view's rows (even)
	static constexpr int LW = (SS_TP + 2*R + 1) & ~1;        // staged width of the reference rows (even)
	static constexpr int NS = WS + 1;                        // row slots of the rings: the window's rows + the next one
	static constexpr int FW = (RW + 4 + 15) & ~15;           // bytes of a staged "full" row piece (dword granules + slack)
	static constexpr int NBMAX = SS_CHUNK/SS_NCB + 1;        // 8-column blocks a pixel can have
	alignas(16) double w[WS][SS_TP][WP];       // LDS image of the windows: [row][pixel][tap]; per tile, a skipped tap's weight -> +0.0
	alignas(16) double rt[NS][RW];             // ring: the other view's rows (NaN: tap unusable)
	alignas(16) double lt[NS][LW];             // ring: the reference rows (NaN: tap unusable)
	alignas(16) double l0[WS][LW];             // the current window's reference rows, NaN -> 0.0 (by window row, not ring slot)
	alignas(16) PixRange pr[2][SS_TP];
	alignas(16) unsigned char full[2][FW];
	unsigned short okm[WS][SS_TP];             // bit col: tap (row, col) of the pixel counts on the reference side
	unsigned short glist[SS_TP*NBMAX];         // select-form work list: pixel*64 + block
	int glist_n;
	int item;
	static_assert(NBMAX <= 64, "work-list entry = pixel*64 + block");
	static_assert(RW % 2 == 0 && LW % 2 == 0 && WP % 2 == 0, "16-byte rows");
	static_assert(RW*8 <= 3*1024, "three pieces per row of the other view");
	static_assert(RW - R + 4 <= SRH_PADR + 1, "padded planes cover every staged piece");
	static_assert(R + 1 <= SRH_PADY, "padded planes cover the rows above and below the image");
};

static_assert(sizeof(SadStripSmem<5>) <= 80*1024 && sizeof(SadStripSmem<2>) <= 80*1024, "two workgroups share a CU's 160 KB of LDS");

// lanes [0, nbytes/16) of the wave copy 16 bytes each from src + 16*lane to LDS dst + 16*lane, 1 KiB per instruction
__device__ __forceinline__ void ss_dma16(const void *src, void *dst, int nbytes, int lane) {
	for (int off = 0; off < nbytes; off += 1024) {
		if (off + lane*16 < nbytes)
			__builtin_amdgcn_global_load_lds((ss_gbl_void *)((const char *)src + off + lane*16),
			                                 (ss_lds_void *)((char *)dst + off), 16, 0, 0);
	}
}
// the same in 4-byte granules (sources that are only 4-byte aligned)
__device__ __forceinline__ void ss_dma4(const void *src, void *dst, int nbytes, int lane) {
	for (int off = 0; off < nbytes; off += 256) {
		if (off + lane*4 < nbytes)
			__builtin_amdgcn_global_load_lds((ss_gbl_void *)((const char *)src + off + lane*4),
			                                 (ss_lds_void *)((char *)dst + off), 4, 0, 0);
	}
}

// One 8-column block of pixel `pi` in the select form (the select form of twoview_rows_sad_kernel, the rows taken from
// the rings): every tap guarded, a skipped tap adds +0.0, numPixels and totalWeight per candidate.  Candidates whose bit
// is set in `store` are written.  (S.w holds the weight itself wherever the reference side counts.)
template <int R>
__device__ __forceinline__ void sad_strip_select_block(const SadStripSmem<R> &S, int s0, int pi, int rc, unsigned store,
                                                    double *__restrict__ dst, double bad_ret, double mcd)
{
	typedef SadStripSmem<R> Smem;
	constexpr int WS = Smem::WS, NS = Smem::NS, NCB = SS_NCB, NR = NCB + 2*R;
	double s[NCB], t[NCB];
	int np[NCB];
#pragma unroll
	for (int j = 0; j < NCB; ++j) { s[j] = 0.0; t[j] = 0.0; np[j] = 0; }
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const unsigned okm = S.okm[row][pi];
		if (okm == 0) continue;                                // (no tap of this window row counts: every term a skipped +0.0)
		const int sl = s0 + row >= NS ? s0 + row - NS : s0 + row;
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
		if ((store >> j) & 1u) dst[(ptrdiff_t)j*SS_TP] = (np[j] <= 4 || t[j] <= 1e-10) ? bad_ret : s[j] / t[j];
}

template <int R>
__global__ __launch_bounds__(SS_NT, 2)
void twoview_strip_sad_kernel(const SadStripArgs A)
{
	typedef SadStripSmem<R> Smem;
	constexpr int WS = Smem::WS, WP = Smem::WP, WPIX = Smem::WPIX, RW = Smem::RW, LW = Smem::LW, NS = Smem::NS;
	constexpr int NCB = SS_NCB, CHUNK = SS_CHUNK, G = SS_G, NT = SS_NT;
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
	const int tiles_per_row = (W + SS_TP - 1)/SS_TP;
	const int SP = padded_stride(W);
	const double mcd = A.max_color_diff;
	const bool fast_ok = mcd == mcd;             // (fmin and the reference's select agree for any non-NaN bound; srh_sad.hip)
	unsigned n_dev = 0;

	for (;;) {
		// ---- next work item: (row segment, tile column); tall segments first, so the tail of the launch is short
		if (tid == 0) S.item = (int)atomicAdd(&A.cnt->strip_ticket, 1u);
		__syncthreads();                           // also: every wave has left the previous item's last tile
		const int item = __builtin_amdgcn_readfirstlane(S.item);
		if (item >= A.nitems) break;
		const int seg = item / tiles_per_row, tx = item - seg*tiles_per_row;
		int ya, nh;
		{
			const int s16 = A.n1 >> 4, s8 = (A.n2 - A.n1) >> 3;
			if (seg < s16) { ya = seg*16; nh = 16; }
			else if (seg < s16 + s8) { ya = A.n1 + (seg - s16)*8; nh = 8; }
			else { ya = A.n2 + (seg - s16 - s8)*4; nh = 4; }
			if (ya + nh > A.nrows) nh = A.nrows - ya;
		}
		const int x0 = tx*SS_TP;
		const int x = x0 + i;
		int cs = 0, rowbase = 0;                   // staging origin (column, even) and the image row held by slot 0

		// one tile's own inputs (nothing here depends on the staging origin): ranges, windows
		auto issue_tile_inputs = [&](int r, int buf, bool ranges, bool windows) {
			const size_t px0 = (size_t)r*W + x0;
			if (ranges && wv == 1) ss_dma4(A.prange + px0, &S.pr[buf][0], SS_TP*8, lane);
			if (windows) {
				// each wave its own pixels' windows (8 pixels x WP taps of every window row): nobody else touches them
				// outside the select form
				const double *wt = A.wimg + ((size_t)r*tiles_per_row + tx)*(size_t)(SS_TP*WPIX);
				for (int a = 0; a < WS; ++a)
					ss_dma16(wt + (size_t)a*(SS_TP*WP) + wv*8*WP, &S.w[a][wv*8][0], 8*WP*8, lane);
			}
		};
		// image row `yy` of both views into ring slot `sl`
		auto issue_row = [&](int yy, int sl) {
			const double *src = A.oth_grayp + (size_t)(yy + SRH_PADY)*SP + (cs - R + SRH_PADL);
			if (wv < 3) { if (wv*1024 + lane*16 < RW*8) __builtin_amdgcn_global_load_lds((ss_gbl_void *)((const char *)src + wv*1024 + lane*16),
			                                                                              (ss_lds_void *)((char *)&S.rt[sl][0] + wv*1024), 16, 0, 0); }
			else ss_dma16(A.ref_tvp + (size_t)(yy + SRH_PADY)*SP + (x0 - R + SRH_PADL), &S.lt[sl][0], LW*8, lane);
		};
		// "full" bytes [cs, cs + RW) of row fy, from the 4-byte granule that holds the first one
		auto issue_full = [&](int fy, int fb) {
			const size_t a0 = (size_t)(fy + SRH_PADY)*SP + (size_t)(cs + SRH_PADL);
			if (wv == 3) ss_dma4(A.oth_fullp + (a0 & ~(size_t)3), &S.full[fb][0], (RW + 4 + 3) & ~3, lane);
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
			int cmin, cmax, cmin_raw;
			{
				const int pi = lane & 31;
				const PixRange q = CS.pr[cur][pi];
				int lo = q.lo, hi = q.hi;
				if (x0 + pi >= W) { lo = 0; hi = -1; }
				int mn = hi >= lo ? lo : 2147483647, mx = hi >= lo ? hi : -2147483647;
#pragma unroll
				for (int d = 16; d >= 1; d >>= 1) {
					const int on = __shfl_xor(mn, d, 64), ox = __shfl_xor(mx, d, 64);
					mn = on < mn ? on : mn; mx = ox > mx ? ox : mx;
				}
				cmin_raw = __builtin_amdgcn_readfirstlane(mn);
				cmax = __builtin_amdgcn_readfirstlane(mx);
				cmin = cmin_raw & ~1;
			}
			const bool any = cmin_raw <= cmax;
			// (re)stage the rings when the strip starts or the ranges have moved outside the staged columns
			if (first || (any && (cmin < cs || cmax > cs + CHUNK - 1))) {
				if (!first) __builtin_amdgcn_s_barrier();          // (a restage in mid-strip: nobody reads the rings any more)
				cs = any ? cmin : 0;
				rowbase = y - R;
				for (int rr = 0; rr < WS; ++rr) issue_row(y - R + rr, rr);
				issue_full(y, cur);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__builtin_amdgcn_s_barrier();
			}
			if (any && cmax > cs + CHUNK - 1) {
				// a candidate range wider than the chunk: not this kernel's case (the host falls back)
				if (tid == 0) atomicAdd(&A.cnt->strip_overflow, 1ull);
				cmax = cs + CHUNK - 1;
			}
			first = false;
			const int s0 = (y - R - rowbase) % NS;                   // ring slot of the window's first row

			// ---- the reference side of the tile, once: which taps count (sample() valid, weight above the cut-off); a
			// skipped tap's weight becomes +0.0 and its gray value 0.0, so that it adds 0 * min(|0 - r|, MAX) = +0.0 in
			// the fast form; a bit per tap for the select form.  Each wave its own pixels' windows.
			for (int row = g; row < WS; row += G) {
				const int sl = s0 + row >= NS ? s0 + row - NS : s0 + row;
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
				const int sl = s0 + row >= NS ? s0 + row - NS : s0 + row;
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
			const int foff = (int)(((size_t)(y + SRH_PADY)*SP + (size_t)(cs + SRH_PADL)) & 3);   // first byte inside its granule
			const unsigned char *rfull = &CS.full[cur][foff];

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
				const PixRange q = CS.pr[cur][i];
				e_min = q.lo; e_max = q.hi;
				if (x >= W) { e_min = 0; e_max = -1; }
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
				const int lo = e_min > cs ? e_min : cs;
				const int hi = e_max < cs + CHUNK - 1 ? e_max : cs + CHUNK - 1;
				const int lo_e = lo & ~1;                                // blocks start on even columns (>= cs)
				const int nblocks = hi >= lo ? (hi - lo_e + NCB)/NCB : 0;
				double *crow = A.cost + tile*(size_t)A.cstride*SS_TP + i;
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
							const int sl = s0 + row >= NS ? s0 + row - NS : s0 + row;
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
							if ((vm >> j) & 1u) crow[(size_t)(c0 + j - e_min)*SS_TP] = bad_full ? A.bad_ret : acc[j] / tw;
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
					const PixRange q = CS.pr[cur][pi];
					qlo = q.lo;
					int qhi = q.hi;
					if (x0 + pi >= W) { qlo = 0; qhi = -1; }
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
				for (int p = tid; p < SS_TP*Smem::NBMAX; p += NT) {
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
					                          A.cost + (tile*(size_t)A.cstride)*SS_TP + (ptrdiff_t)(c0 - qlo)*SS_TP + pi,
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

template <int R>
static void launch_sad_strip_variant(hipStream_t st, const SadStripArgs &a, int num_cus)
{
	typedef SadStripSmem<R> Smem;
	const size_t lds = sizeof(Smem);
	(void)hipFuncSetAttribute((const void *)twoview_strip_sad_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	int grid = num_cus*2;
	if (grid > a.nitems) grid = a.nitems;
	if (grid < 1) grid = 1;
	hipLaunchKernelGGL((twoview_strip_sad_kernel<R>), dim3((unsigned)grid), dim3(SS_NT), lds, st, a);
}

bool launch_twoview_strip_sad(hipStream_t st, int width, int height, const srh_params &P, int y0, int nrows,
                              const double *wimg, const PixRange *prange, const double *ref_tvp, const double *oth_grayp,
                              const uint8_t *oth_fullp, double *cost, int cstride, Counters *cnt, int num_cus)
{
	if (SS_CHUNK != strip_chunk_columns()) return false;
	SadStripArgs a;
	a.W = width; a.H = height; a.y0 = y0; a.nrows = nrows;
	a.wimg = wimg; a.prange = prange;
	a.ref_tvp = ref_tvp; a.oth_grayp = oth_grayp; a.oth_fullp = oth_fullp;
	a.cost = cost; a.cstride = cstride; a.cnt = cnt;
	a.weight_cutoff = P.weight_cutoff; a.bad_ret = P.bad_ret; a.max_color_diff = P.max_color_diff;
	sad_strip_items(a);
	switch (P.window_radius) {
	case 5: launch_sad_strip_variant<5>(st, a, num_cus); return true;
	case 2: launch_sad_strip_variant<2>(st, a, num_cus); return true;
	default: return false;
	}
}

} // namespace srh
