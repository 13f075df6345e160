// srh_stripframe.hpp -- the FRAME of the persistent strip kernels of the dense TwoView plan, stated once:
// twoview_strip_cost_kernel (srh_strip.hip, NCC), twoview_strip_sad_kernel (srh_sad_strip.hip, SAD) and
// twoview_strip_census_kernel (srh_census_strip.hip, census) differ in their block loops, select forms and per-tile passes;
// what surrounds those is here.
//
//   padded raster      SRH_PADL / SRH_PADR / SRH_PADY, padded_stride, padded_size, padded_raster_xy (raster index -> image
//                      position and "inside"), padded_raster_kernel + launch_padded_raster: a plane is one functor
//   StripGeom<R>       tile and staging geometry: STRIP_TP / STRIP_NCB / STRIP_CHUNK, widths of the staged rows, ring slots
//   StripItems         the work-item cut of a band (cut, segment) and of its image-border rows (border_rows, cut_border,
//                      segment_border)
//   ring_slot          (s0 + row) mod NS for s0 < NS, row < NS
//   strip_lane_blocks  a lane's block geometry lo, hi, lo_e, nblocks
//   device only        strip_dma16 / strip_dma4, strip_draw_item, strip_pixel_range, tile_range_union, needs_restage,
//                      strip_clamp_to_chunk, full_offset, strip_request_row / _full, launch_strip
//
// The first five are host-clean: the CPU suite compiles them with g++ (tests/stripframe_host.cpp,
// tests/test_stripframe_host.py).  Every device function is force-inlined and takes what it needs by value: how a
// helper is called is part of the kernels' register allocation (profiles/README.md, "Strip frame").
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef SRH_NHD                        // (srh_ncc.hpp, srh_wta.hpp and srh_block.hpp have the same definition)
#if defined(__HIPCC__)
#define SRH_NHD __host__ __device__ __forceinline__
#else
#define SRH_NHD inline
#endif
#endif

namespace srh {

// ------------------------------------------------------------------ padded raster
// NaN-bordered copy of a view's gray_tv plane (and zero-bordered copy of its "window fully usable" plane):
// every row piece a tile stages lies inside the allocation, so the LDS-DMA needs no bounds handling and the
// border taps arrive as NaN (= "tap skipped", vectorimage.cpp:115-119,129-155).
#define SRH_PADL 8
#define SRH_PADR 344          // >= CHUNK + R + NCB + 2 of the strip kernels
#define SRH_PADY 8
SRH_NHD int padded_stride(int w) { return w + SRH_PADL + SRH_PADR; }
SRH_NHD size_t padded_size(int w, int h) { return (size_t)padded_stride(w)*(size_t)(h + 2*SRH_PADY); }
// candidate column range of a reference pixel on its own row of the other view (empty: hi < lo)
struct PixRange { int32_t lo, hi; };

// raster index k < padded_size(W, H) -> the image position it stands for; true inside the W x H image, whose pixel (x, y)
// is at (y + SRH_PADY)*padded_stride(W) + x + SRH_PADL
SRH_NHD bool padded_raster_xy(size_t k, int W, int H, int &x, int &y) {
	const size_t SP = (size_t)padded_stride(W);
	x = (int)(k % SP) - SRH_PADL; y = (int)(k / SP) - SRH_PADY;
	return x >= 0 && y >= 0 && x < W && y < H;
}

// ------------------------------------------------------------------ tile and staging geometry
constexpr int STRIP_TP = 32;                   // pixels per tile (= SRH_WTILE)
constexpr int STRIP_NCB = 8;                   // candidate columns per block
constexpr int STRIP_CHUNK = 320;               // candidate columns a tile can hold in LDS (strip_chunk_columns())
constexpr int STRIP_BROWS = 1;                 // rows per work item of the NCC kernel's border instantiation

template <int R>
struct StripGeom {
	static constexpr int WS = 2*R + 1;
	static constexpr int WP = (WS + 1) & ~1;                       // taps per window row, padded even
	static constexpr int WPIX = WS*WP;                             // doubles per pixel window
	static constexpr int RW = STRIP_CHUNK + 2*R + STRIP_NCB + 2;   // staged width of the other view's rows (even)
	static constexpr int LW = (STRIP_TP + 2*R + 1) & ~1;           // staged width of the reference rows (even)
	static constexpr int NS = WS + 1;                              // row slots of the rings: the window's rows + the next one
	static constexpr int FW = (RW + 4 + 15) & ~15;                 // bytes of a staged "full" row piece (dword granules + slack)
	static constexpr int NBMAX = STRIP_CHUNK/STRIP_NCB + 1;        // 8-column blocks a pixel can have
	static_assert(RW % 2 == 0 && LW % 2 == 0 && WP % 2 == 0, "16-byte rows");
	static_assert(RW*8 <= 3*1024, "three pieces per row of the other view");
	static_assert(RW - R + 4 <= SRH_PADR + 1, "padded planes cover every staged piece");
	static_assert(R + 1 <= SRH_PADY, "padded planes cover the rows above and below the image");
};

// ring slot of window row `row` when the window's first row is in slot s0 (s0 < NS, row < NS)
SRH_NHD int ring_slot(int s0, int row, int NS) { return s0 + row >= NS ? s0 + row - NS : s0 + row; }

// ------------------------------------------------------------------ work items
// A band's rows, tall items first, so the tail of a launch is short: 3/4 of the rows in 16-row items, 2/3 of the rest in
// 8-row items, the remainder in 4-row items; item = segment*tiles_per_row + tile column.
// The NCC kernel's border instantiation works the rows [0, t) and [b, nrows) whose window the image's top or bottom edge
// cuts, in items of up to STRIP_BROWS rows, tile column major with the two edge columns first (their corner pixels leave
// the most to phase 2, so they should not be the launch's last items): n1 = t, n2 = b.
struct StripItems {
	int n1, n2;                             // rows [0,n1) in 16-row items, [n1,n2) in 8-row items, the rest in 4-row items
	int nitems;

	static inline StripItems cut(int nrows, int W) {
		StripItems s;
		s.n1 = ((nrows*3/4)/16)*16;
		s.n2 = s.n1 + (((nrows - s.n1)*2/3)/8)*8;
		const int nseg = s.n1/16 + (s.n2 - s.n1)/8 + (nrows - s.n2 + 3)/4;
		s.nitems = nseg*((W + STRIP_TP - 1)/STRIP_TP);
		return s;
	}
	// item -> tile column tx, band rows [ya, ya + nh)
	SRH_NHD void segment(int item, int tiles_per_row, int nrows, int &tx, int &ya, int &nh) const {
		const int seg = item / tiles_per_row;
		tx = item - seg*tiles_per_row;
		const int s16 = n1 >> 4, s8 = (n2 - n1) >> 3;
		if (seg < s16) { ya = seg*16; nh = 16; }
		else if (seg < s16 + s8) { ya = n1 + (seg - s16)*8; nh = 8; }
		else { ya = n2 + (seg - s16 - s8)*4; nh = 4; }
		if (ya + nh > nrows) nh = nrows - ya;
	}

	// rows [0, t) and [b, nrows) of the band [y0, y0 + nrows) of an image of H rows: y < R or y > H - 2 - R
	static inline void border_rows(int y0, int nrows, int H, int R, int &t, int &b) {
		t = R - y0; if (t < 0) t = 0; if (t > nrows) t = nrows;
		b = H - 1 - R - y0; if (b < t) b = t; if (b > nrows) b = nrows;
	}
	static inline StripItems cut_border(int t, int b, int nrows, int W) {
		StripItems s;
		s.n1 = t; s.n2 = b;
		s.nitems = ((t + STRIP_BROWS - 1)/STRIP_BROWS + (nrows - b + STRIP_BROWS - 1)/STRIP_BROWS)*((W + STRIP_TP - 1)/STRIP_TP);
		return s;
	}
	SRH_NHD void segment_border(int item, int tiles_per_row, int nrows, int &tx, int &ya, int &nh) const {
		const int st = (n1 + STRIP_BROWS - 1)/STRIP_BROWS, nseg = st + (nrows - n2 + STRIP_BROWS - 1)/STRIP_BROWS;
		const int k = item / nseg, seg = item - k*nseg;
		tx = k == 0 ? 0 : k == 1 ? tiles_per_row - 1 : k - 1;
		if (seg < st) { ya = seg*STRIP_BROWS; nh = n1 - ya; }
		else { ya = n2 + (seg - st)*STRIP_BROWS; nh = nrows - ya; }
		if (nh > STRIP_BROWS) nh = STRIP_BROWS;
	}
};

// ------------------------------------------------------------------ a lane's blocks
// The pixel's range [e_min, e_max] cut to the staged columns [cs, cs + CHUNK): [lo, hi]; its blocks of NCB columns start
// at lo_e -- on an even column (>= cs: cs is even) where the rows are read 16 bytes at a time (PAD), else at lo itself.
template <bool PAD>
SRH_NHD void strip_lane_blocks(int e_min, int e_max, int cs, int &lo, int &hi, int &lo_e, int &nblocks) {
	lo = e_min > cs ? e_min : cs;
	hi = e_max < cs + STRIP_CHUNK - 1 ? e_max : cs + STRIP_CHUNK - 1;
	lo_e = PAD ? (lo & ~1) : lo;
	nblocks = hi >= lo ? (hi - lo_e + STRIP_NCB)/STRIP_NCB : 0;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------ padded planes
// out[k] = value(x, y, inside) over the padded raster of a W x H image
template <class T, class F>
__global__ void padded_raster_kernel(int W, int H, T *__restrict__ out, F value)
{
	const size_t n = padded_size(W, H);
	for (size_t k = (size_t)blockIdx.x*blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x*blockDim.x) {
		int x, y;
		const bool in = padded_raster_xy(k, W, H, x, y);
		out[k] = value(x, y, in);
	}
}
template <class T, class F>
static void launch_padded_raster(hipStream_t st, int w, int h, T *out, F value) {
	size_t n = padded_size(w, h);
	size_t b = (n + 255)/256; if (b > 4096) b = 4096;
	hipLaunchKernelGGL((padded_raster_kernel<T, F>), dim3((unsigned)b), dim3(256), 0, st, w, h, out, value);
}

// ------------------------------------------------------------------ LDS-DMA
typedef __attribute__((address_space(3))) void strip_lds_void;
typedef __attribute__((address_space(1))) const void strip_gbl_void;

// lanes [0, nbytes/16) of the wave copy 16 bytes each from src + 16*lane to LDS dst + 16*lane, 1 KiB per instruction
__device__ __forceinline__ void strip_dma16(const void *src, void *dst, int nbytes, int lane) {
	for (int off = 0; off < nbytes; off += 1024) {
		if (off + lane*16 < nbytes)
			__builtin_amdgcn_global_load_lds((strip_gbl_void *)((const char *)src + off + lane*16),
			                                 (strip_lds_void *)((char *)dst + off), 16, 0, 0);
	}
}
// the same in 4-byte granules (sources that are only 4-byte aligned)
__device__ __forceinline__ void strip_dma4(const void *src, void *dst, int nbytes, int lane) {
	for (int off = 0; off < nbytes; off += 256) {
		if (off + lane*4 < nbytes)
			__builtin_amdgcn_global_load_lds((strip_gbl_void *)((const char *)src + off + lane*4),
			                                 (strip_lds_void *)((char *)dst + off), 4, 0, 0);
	}
}

// ------------------------------------------------------------------ the tile frame
// next work item from the ticket counter, through the LDS word `slot`; the barrier also says that every wave has left
// the previous item's last tile
__device__ __forceinline__ int strip_draw_item(unsigned int *ticket, int *slot, int tid) {
	if (tid == 0) *slot = (int)atomicAdd(ticket, 1u);
	__syncthreads();
	return __builtin_amdgcn_readfirstlane(*slot);
}

// a pixel's candidate range; empty outside the image
__device__ __forceinline__ void strip_pixel_range(const PixRange q, bool inside, int &lo, int &hi) {
	lo = q.lo; hi = q.hi;
	if (!inside) { lo = 0; hi = -1; }
}

// Union of the tile's 32 candidate ranges: lanes k and k + 32 hold pixel k's [lo, hi] (empty: hi < lo).  Every wave works
// it out for itself, within each row of 16 lanes by DPP rotations -- four steps, no LDS -- and the two rows by lane reads
// (as five butterfly steps of ds_bpermute each reduction was five dependent LDS round trips).  Empty: cmin_raw > cmax.
__device__ __forceinline__ void tile_range_union(int lo, int hi, int &cmin_raw, int &cmax) {
	int mn = hi >= lo ? lo : 2147483647, mx = hi >= lo ? hi : -2147483647;
#define SRH_ROR(v, n) __builtin_amdgcn_update_dpp(0, (v), 0x120 + (n), 0xf, 0xf, false)
#pragma unroll
	for (int d = 8; d >= 1; d >>= 1) {
		const int on = d == 8 ? SRH_ROR(mn, 8) : d == 4 ? SRH_ROR(mn, 4) : d == 2 ? SRH_ROR(mn, 2) : SRH_ROR(mn, 1);
		const int ox = d == 8 ? SRH_ROR(mx, 8) : d == 4 ? SRH_ROR(mx, 4) : d == 2 ? SRH_ROR(mx, 2) : SRH_ROR(mx, 1);
		mn = on < mn ? on : mn; mx = ox > mx ? ox : mx;
	}
#undef SRH_ROR
	const int m0 = __builtin_amdgcn_readlane(mn, 0), m1 = __builtin_amdgcn_readlane(mn, 16);
	const int x0 = __builtin_amdgcn_readlane(mx, 0), x1 = __builtin_amdgcn_readlane(mx, 16);
	cmin_raw = m0 < m1 ? m0 : m1;
	cmax = x0 > x1 ? x0 : x1;
}

// (re)stage the rings when the strip starts or the ranges have moved outside the staged columns [cs, cs + CHUNK)
__device__ __forceinline__ bool needs_restage(bool first, bool any, int cmin, int cmax, int cs) {
	return first || (any && (cmin < cs || cmax > cs + STRIP_CHUNK - 1));
}

// a candidate range wider than the chunk: not these kernels' case (the host falls back on the counter)
__device__ __forceinline__ void strip_clamp_to_chunk(bool any, int cs, int &cmax, int tid, unsigned long long *overflow) {
	if (any && cmax > cs + STRIP_CHUNK - 1) {
		if (tid == 0) atomicAdd(overflow, 1ull);
		cmax = cs + STRIP_CHUNK - 1;
	}
}

// the staged "full" bytes start at the 4-byte granule that holds column cs of row y: the first byte's place inside it
__device__ __forceinline__ int full_offset(int y, int SP, int cs) {
	return (int)(((size_t)(y + SRH_PADY)*SP + (size_t)(cs + SRH_PADL)) & 3);
}

// Requests, by wave role.  Image row `yy` of both views into one ring slot: waves 0-2 a 1 KiB piece each of the other view's
// row from column cs - R, wave 3 the reference row from column x0 - R.
// (T: the planes' 8-byte word -- gray values, or the census kernel's signatures)
template <int R, class T>
__device__ __forceinline__ void strip_request_row(const T *othp, const T *refp, int SP, int yy, int cs, int x0,
                                                  T *rt, T *lt, int wv, int lane) {
	static_assert(sizeof(T) == 8, "rows of 8-byte words");
	const T *src = othp + (size_t)(yy + SRH_PADY)*SP + (cs - R + SRH_PADL);
	if (wv < 3) {
		if (wv*1024 + lane*16 < StripGeom<R>::RW*8)
			__builtin_amdgcn_global_load_lds((strip_gbl_void *)((const char *)src + wv*1024 + lane*16),
			                                 (strip_lds_void *)((char *)rt + wv*1024), 16, 0, 0);
	}
	else if (wv == 3) strip_dma16(refp + (size_t)(yy + SRH_PADY)*SP + (x0 - R + SRH_PADL), lt, StripGeom<R>::LW*8, lane);
}
// "full" bytes [cs, cs + RW) of row fy, from the 4-byte granule that holds the first one (one wave's: the caller says which)
template <int R>
__device__ __forceinline__ void strip_request_full(const uint8_t *fullp, int SP, int fy, int cs, unsigned char *dst, int lane) {
	const size_t a0 = (size_t)(fy + SRH_PADY)*SP + (size_t)(cs + SRH_PADL);
	strip_dma4(fullp + (a0 & ~(size_t)3), dst, (StripGeom<R>::RW + 4 + 3) & ~3, lane);
}
// (The tile's 32 candidate ranges are wave 1's, one strip_dma4 in each kernel's own request of the tile's inputs: as a
// function of this header that line moved the NCC kernel's register allocation, profiles/README.md.)

// ------------------------------------------------------------------ launch
// `lds` bytes of dynamic LDS; one workgroup per work item up to what the device holds at once
template <class Args>
static void launch_strip(hipStream_t st, void (*kernel)(const Args), const Args &a, size_t lds, int threads, int wg_per_cu,
                         int num_cus, int nitems)
{
	(void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	int grid = num_cus*wg_per_cu;
	if (grid > nitems) grid = nitems;
	if (grid < 1) grid = 1;
	hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, st, a);
}
#endif  // __HIPCC__

}  // namespace srh
