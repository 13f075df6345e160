// srh_filter.hpp -- the per-element pieces of TwoViewStereo::filterInvalidPixels (stereo/twoviewstereo.cpp:676-811) and
// weightedMedian (:821-860), usable from host and gfx950 device code: srh_filter.hip runs them per pixel / per hole, and
// the CPU suite compiles this header with g++ and holds it against std::make_heap / std::pop_heap and the loop of the
// reference (tests/test_filter_host.py).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SRH_FHD __host__ __device__ __forceinline__
#else
#define SRH_FHD inline
#endif

namespace srh {
namespace filt {

SRH_FHD bool is_inf(double v) { return v == HUGE_VAL || v == -HUGE_VAL; }         // std::isinf
SRH_FHD bool is_nan(double v) { return !(v == v); }
SRH_FHD bool is_fin(double v) { return fabs(v) <= 1.7976931348623157e308; }       // std::isfinite

// ---- gap fill (the compiled body of filterInvalidPixels, :682-767), one pixel of one row ----------------------------
// The reference walks a row left to right.  A run [start, end] of isinf pixels is filled when end - start < gap; its
// left value is the row's pixel before the run (at the row start: pixel 0 itself, an inf, which then takes the right
// value), its right value the pixel after the run (NaN past the row's end); a non-finite one of the two takes the
// other's value; the run is written from both ends inward, one pixel from each end per step, the right end second.
// So pixel x of the run ends up with the left value when x - start < end - x and with the right value otherwise (the
// middle pixel of an odd run: right).  The fills only touch pixels left of the scan position, so the reference reads the
// original row throughout, and every pixel can be decided on its own from the run it lies in -- which is what this
// does.  A scan stops after gap + 1 pixels each way: a run that long is not filled.  Returns true (and *out) when x is
// filled; otherwise *out = row[x].
SRH_FHD bool gap_fill_pixel(const double *row, int w, int x, int gap, double *out)
{
	*out = row[x];
	if (!is_inf(row[x]) || gap <= 0) return false;
	int s = x, e = x;
	while (s > 0 && is_inf(row[s - 1]) && x - s <= gap) --s;
	while (e + 1 < w && is_inf(row[e + 1]) && e - s < gap) ++e;
	if (e - s >= gap) return false;
	double l = s > 0 ? row[s - 1] : row[0];
	double r = e + 1 < w ? row[e + 1] : (double)NAN;
	if (!is_fin(l)) l = r;
	if (!is_fin(r)) r = l;
	*out = (x - s < e - x) ? l : r;
	return true;
}

// ---- weightedMedian's selection, replayed exactly ------------------------------------------------------------------
// The kept taps (depth not NaN, inside [min_depth, max_depth], weight > 1e-10) go into a heap in the order they were
// kept (row-major); std::make_heap / std::pop_heap of libstdc++ (bits/stl_heap.h: __make_heap, __adjust_heap,
// __push_heap, __pop_heap) order them by depth alone (comparePairFirst), so which of equal depths pops first depends on
// this exact sequence of moves -- and the float sums weight1 / totalWeights on the order of the pops.  The heap holds tap
// indices h[i*hs] (stride hs: one lane's column of an LDS array on the device, 1 on the host); key(t) is tap t's depth.
template <class Key>
SRH_FHD void heap_push_up(uint8_t *h, int hs, int hole, int top, uint8_t v, Key key)
{
	int parent = (hole - 1) / 2;
	const double kv = key(v);
	while (hole > top && key(h[parent*hs]) < kv) {
		h[hole*hs] = h[parent*hs];
		hole = parent;
		parent = (hole - 1) / 2;
	}
	h[hole*hs] = v;
}

template <class Key>
SRH_FHD void heap_adjust(uint8_t *h, int hs, int hole, int len, uint8_t v, Key key)
{
	const int top = hole;
	int second = hole;
	while (second < (len - 1) / 2) {
		second = 2*(second + 1);
		if (key(h[second*hs]) < key(h[(second - 1)*hs])) second--;
		h[hole*hs] = h[second*hs];
		hole = second;
	}
	if ((len & 1) == 0 && second == (len - 2) / 2) {
		second = 2*(second + 1);
		h[hole*hs] = h[(second - 1)*hs];
		hole = second - 1;
	}
	heap_push_up(h, hs, hole, top, v, key);
}

template <class Key>
SRH_FHD void heap_make(uint8_t *h, int hs, int len, Key key)
{
	if (len < 2) return;
	for (int parent = (len - 2) / 2; ; --parent) {
		heap_adjust(h, hs, parent, len, h[parent*hs], key);
		if (parent == 0) return;
	}
}

// std::pop_heap(h, h + len): the largest moves to h[len - 1]
template <class Key>
SRH_FHD void heap_pop(uint8_t *h, int hs, int len, Key key)
{
	if (len < 2) return;
	const uint8_t v = h[(len - 1)*hs];
	h[(len - 1)*hs] = h[0];
	heap_adjust(h, hs, 0, len - 1, v, key);
}

// The loop of weightedMedian after the taps are kept: n kept tap indices in h, their weights summed (in keeping order)
// to `total`.  Returns the median depth (NaN when fewer than 2 taps are kept or total <= 1e-10).
template <class Key, class Wt>
SRH_FHD double weighted_median_replay(uint8_t *h, int hs, int n, double total, Key key, Wt wt)
{
	double ret = (double)NAN;
	if (!(n > 1 && total > 1e-10)) return ret;
	heap_make(h, hs, n, key);
	double weight1 = 0.0;
	int len = n;
	while (weight1 < total && len > 0) {          // (len > 0: the sums end the loop first; the reference has no guard)
		heap_pop(h, hs, len, key);
		const uint8_t t = h[(len - 1)*hs];
		const double w = wt(t);
		weight1 += w;
		total -= w;
		ret = key(t);
		--len;
	}
	return ret;
}

}  // namespace filt
}  // namespace srh
