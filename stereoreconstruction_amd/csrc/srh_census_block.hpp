// srh_census_block.hpp -- the BLOCKS of the support-weighted census cost on the dense plan (twoview_strip_census_kernel,
// srh_census_strip.hip), stated once and usable from host and gfx950 device code: the per-tile settle of the
// reference side, the fast-form and the select-form sums of a block of adjacent candidates, and the finish.  The kernel
// calls them with a ROW SOURCE that says where a window row comes from (its LDS rings); the CPU suite compiles this header
// with g++ and holds it to cost_census of tests/census_restatement.cpp (tests/census_block_host.cpp,
// tests/test_census_block_host.py).
//
//   CENSUS_UNUSABLE       the word of a tap that does not count: bits 31 and 63 of a signature are always 0, so bit 63 marks
//   census_usable         the tap's word is a signature
//   census_distance       Hamming distance of two signatures
//   census_settle_row     one window row of a reference pixel: a skipped tap's weight becomes +0.0, a bit per counting tap
//   census_pixel_totals   totalWeight and numPixels of the pixel when the other side is fully usable
//   census_fast_block     sums of NC adjacent candidates whose windows in the other view are fully usable
//   census_select_block   sum, totalWeight, numPixels of NCB adjacent candidates, every tap guarded
//   census_finish         bad_ret, or sum / totalWeight
//
// A row source is a struct with one forceinline member, `CensusRow row(int row) const`: where window row `row` of the
// pixel and of the block's first candidate start.
//
// These are the sums of tv_cost_census (srh_walk.hpp) in its order: taps row-major, one fused multiply-add per counting
// tap.  A tap the reference side skips carries the weight +0.0 and leaves a sum as it is (every term is >= 0 and the sums
// start at +0.0): the argument of srh_census.hip.  Fused only where __builtin_fma is written: build without contraction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef SRH_NHD                        // (srh_ncc.hpp, srh_wta.hpp, srh_block.hpp and srh_stripframe.hpp have the same definition)
#if defined(__HIPCC__)
#define SRH_NHD __host__ __device__ __forceinline__
#else
#define SRH_NHD inline
#endif
#endif

namespace srh {

constexpr uint64_t CENSUS_UNUSABLE = (uint64_t)1 << 63;

SRH_NHD bool census_usable(uint64_t word) { return (int64_t)word >= 0; }
// (the two halves counted as 32-bit words: the sum converts to a double in one instruction; a 64-bit count's convert is
// two -- a convert and an addition of the upper half's +0.0)
SRH_NHD int census_distance(uint64_t a, uint64_t b) {
	const uint64_t d = a ^ b;
	return __builtin_popcount((uint32_t)d) + __builtin_popcount((uint32_t)(d >> 32));
}

// One window row of a pixel and a block: r = the other view's words from the first candidate's left tap on (16-byte
// aligned: blocks start on even columns of rings that do), w = the row's weights, l = the reference view's words from the
// pixel's left tap on, okm = bit col: the reference side counts tap col (census_settle_row)
struct CensusRow { const uint64_t *r; const double *w; const uint64_t *l; unsigned okm; };

// the reference side of one window row, settled in place: tap col counts iff its word is a signature and its weight is above
// the cut-off; a skipped tap's weight becomes +0.0.  Returns the row's bits.
template <int WS>
SRH_NHD unsigned census_settle_row(const uint64_t *l, double *w, double weight_cutoff) {
	unsigned m = 0;
#pragma unroll
	for (int col = 0; col < WS; ++col) {
		const double wt = w[col];
		const bool okl = census_usable(l[col]) && wt > weight_cutoff;
		w[col] = okl ? wt : 0.0;
		m |= okl ? 1u << col : 0u;
	}
	return m;
}

// totalWeight and numPixels of a settled pixel whose candidate's window is fully usable: the reference's additions in its
// order (a skipped tap adds +0.0)
template <int WS, class Src>
SRH_NHD void census_pixel_totals(const Src src, double &tw, int &npx) {
	tw = 0.0; npx = 0;
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const CensusRow q = src.row(row);
#pragma unroll
		for (int col = 0; col < WS; ++col) tw += q.w[col];
		npx += __builtin_popcount(q.okm);
	}
}

// the other view's segment of N words (N even) from a 16-byte aligned start
template <int N>
SRH_NHD void census_load_segment(const uint64_t *r, uint64_t (&rr)[N]) {
	static_assert(N % 2 == 0, "16-byte rows");
	const uint64_t *ra = (const uint64_t *)__builtin_assume_aligned(r, 16);
#pragma unroll
	for (int m = 0; m < N; ++m) rr[m] = ra[m];
}

// fast form: acc[j] = the sum of candidate j of the block, j < NC; every tap of the other side is a signature
template <int WS, int NC, class Src>
SRH_NHD void census_fast_block(const Src src, double (&out)[NC]) {
	constexpr int NRC = NC + WS - 1;
	double acc[NC];
#pragma unroll
	for (int j = 0; j < NC; ++j) acc[j] = 0.0;
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const CensusRow q = src.row(row);
		uint64_t rr[NRC];
		census_load_segment<NRC>(q.r, rr);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const double we = q.w[col];
			const uint64_t sg = q.l[col];
#pragma unroll
			for (int j = 0; j < NC; ++j) acc[j] = __builtin_fma(we, (double)census_distance(sg, rr[col + j]), acc[j]);
		}
	}
#pragma unroll
	for (int j = 0; j < NC; ++j) out[j] = acc[j];
}

// select form: every tap guarded on both sides; a skipped tap adds +0.0 to the two sums and nothing to numPixels
template <int WS, int NCB, class Src>
SRH_NHD void census_select_block(const Src src, double (&sum)[NCB], double (&tw)[NCB], int (&npx)[NCB]) {
	constexpr int NR = NCB + WS - 1;
	double s[NCB], t[NCB];
	int np[NCB];
#pragma unroll
	for (int j = 0; j < NCB; ++j) { s[j] = 0.0; t[j] = 0.0; np[j] = 0; }
#pragma unroll 1
	for (int row = 0; row < WS; ++row) {
		const CensusRow q = src.row(row);
		if (q.okm == 0) continue;                                  // (no tap of this window row counts: every term a skipped +0.0)
		uint64_t rr[NR];
		census_load_segment<NR>(q.r, rr);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const double wt = q.w[col];
			const uint64_t sg = q.l[col];
			const bool okl = (q.okm >> col) & 1u;
#pragma unroll
			for (int j = 0; j < NCB; ++j) {
				const bool ok = okl && census_usable(rr[col + j]);
				const double we = ok ? wt : 0.0;
				s[j] = __builtin_fma(we, (double)census_distance(sg, rr[col + j]), s[j]);
				t[j] += we;
				np[j] += ok ? 1 : 0;
			}
		}
	}
#pragma unroll
	for (int j = 0; j < NCB; ++j) { sum[j] = s[j]; tw[j] = t[j]; npx[j] = np[j]; }
}

SRH_NHD double census_finish(int numPixels, double totalWeight, double sum, double bad_ret) {
	return (numPixels <= 4 || totalWeight <= 1e-10) ? bad_ret : sum / totalWeight;
}

}  // namespace srh
