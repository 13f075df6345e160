// filter_restatement.cpp -- CPU restatement of TwoViewStereo::filterInvalidPixels (stereo/twoviewstereo.cpp:676-811,
// with its #if 0 half) and weightedMedian (:821-860) for one map, written as the reference's loops are, with the real
// std::make_heap / std::pop_heap of this compiler and the oracle's sro_weights for the support windows.  Built at test
// time as a shared library (tests/test_filter_host.py) and loaded with ctypes.
//
// Besides the restatement it exports two checks of the library's device header srh_filter.hpp compiled for the host:
// its per-pixel gap fill against the row loop, and its heap replay against std::pop_heap.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "sr_oracle.h"
#include "srh_filter.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN();
const double INF = std::numeric_limits<double>::infinity();

// the compiled body of filterInvalidPixels (:685-725), one map of w x h
void gapFill(std::vector<double> &d, int w, int h, int gapWidth) {
	for (int y = 0; y < h; ++y) {
		double *row = d.data() + static_cast<size_t>(y)*w;
		for (int x = 0; x < w;) {
			double ldepth = row[x];
			while (x < w && !std::isinf(row[x])) {
				ldepth = row[x];
				++x;
			}
			if (x >= w)
				continue;
			double rdepth = INF;
			int start = x;
			while (x < w && std::isinf(row[x])) {
				rdepth = row[x];
				++x;
			}
			if (x < w)
				rdepth = row[x];
			else
				rdepth = NaN;
			int end = x - 1;
			if (end - start < gapWidth) {
				if (!std::isfinite(ldepth)) ldepth = rdepth;
				if (!std::isfinite(rdepth)) rdepth = ldepth;
				while (start <= end) {
					row[start] = ldepth;
					row[end] = rdepth;
					++start;
					--end;
				}
			}
		}
	}
}

typedef std::pair<double, double> ValuePair;

bool comparePairFirst(const ValuePair &a, const ValuePair &b) { return a.first < b.first; }

// weightedMedian (:821-860); weights = the window of (x, y), row-major.  Taps outside the map are skipped (their weight
// is 0 in the reference, which reads a wrapped row or past the map there).
double weightedMedian(const std::vector<double> &depths, int w, int h, int x, int y, const double *weights, int R,
                      double minDepth, double maxDepth) {
	const int WS = 2*R + 1;
	std::vector<ValuePair> vals;
	vals.reserve(WS*WS);
	double totalWeights = 0.0;
	for (int row = -R; row <= R; ++row) {
		for (int col = -R; col <= R; ++col) {
			const int xt = x + col;
			const int yt = y + row;
			if (xt < 0 || yt < 0 || xt >= w || yt >= h) continue;
			const double depth = depths[static_cast<size_t>(yt)*w + xt];
			if (std::isnan(depth) || depth < minDepth || depth > maxDepth)
				continue;
			const double weight = weights[(row + R)*WS + (col + R)];
			if (weight > 1e-10) {
				vals.push_back(ValuePair(depth, weight));
				totalWeights += weight;
			}
		}
	}
	double ret = NaN;
	if (vals.size() > 1 && totalWeights > 1e-10) {
		std::make_heap(vals.begin(), vals.end(), comparePairFirst);
		double weight1 = 0.0;
		while (weight1 < totalWeights && !vals.empty()) {
			std::pop_heap(vals.begin(), vals.end(), comparePairFirst);
			weight1 += vals.back().second;
			totalWeights -= vals.back().second;
			ret = vals.back().first;
			vals.pop_back();
		}
	}
	return ret;
}

}  // namespace

extern "C" {

// out = filterInvalidPixels(D) for one map; flags: 1 gap fill, 2 weighted median (srh_view_filter_invalid's contract)
void fr_filter(const sro_image *img, const sro_params *p, const double *D, double *out, int flags, int gapWidth) {
	const int w = img->w, h = img->h, R = p->window_radius, WS = 2*R + 1;
	const size_t n = static_cast<size_t>(w)*h;
	std::vector<double> G(D, D + n), copy(D, D + n);
	if (flags & 1) gapFill(G, w, h, gapWidth);
	if (!(flags & 2)) { std::memcpy(out, G.data(), n*sizeof(double)); return; }
	std::vector<double> weights(WS*WS);
	for (int y = 0; y < h; ++y)
		for (int x = 0; x < w; ++x) {
			const size_t i = static_cast<size_t>(y)*w + x;
			if (img->mask && img->mask[i] != 1) {
				copy[i] = NaN;
				continue;
			}
			if (!std::isfinite(copy[i])) {
				sro_weights(img, x, y, p, weights.data());
				copy[i] = weightedMedian(G, w, h, x, y, weights.data(), R, p->min_depth, p->max_depth);
			}
		}
	std::memcpy(out, copy.data(), n*sizeof(double));
}

// the median of one window (weights row-major, depths = the window's depths, NaN off the map)
double fr_weighted_median(const double *depths, const double *weights, int R, double minDepth, double maxDepth) {
	const int WS = 2*R + 1;
	std::vector<double> d(depths, depths + WS*WS);
	return weightedMedian(d, WS, WS, R, R, weights, R, minDepth, maxDepth);
}

// the library's per-pixel gap fill (srh_filter.hpp) over one map
void fr_lib_gap_fill(const double *D, double *out, int w, int h, int gapWidth) {
	for (int y = 0; y < h; ++y)
		for (int x = 0; x < w; ++x)
			srh::filt::gap_fill_pixel(D + static_cast<size_t>(y)*w, w, x, gapWidth, out + static_cast<size_t>(y)*w + x);
}

// the library's replay (srh_filter.hpp) against std::make_heap / std::pop_heap: `trials` random tie-heavy sets of 2..121
// (depth, weight) pairs; every pop of the whole heap must give the same (depth, original index), and the library's
// weighted_median_replay the bits of weightedMedian's loop.  Returns the number of trials that differ.
int fr_heap_check(unsigned seed, int trials) {
	std::mt19937 rng(seed);
	int bad = 0;
	for (int trial = 0; trial < trials; ++trial) {
		const int n = 2 + static_cast<int>(rng() % 120);
		const int distinct = 1 + static_cast<int>(rng() % (trial % 3 == 0 ? 3 : 40));
		std::vector<double> depth(n), weight(n);
		for (int i = 0; i < n; ++i) {
			depth[i] = 1.0 + static_cast<double>(rng() % distinct)*0.25;
			weight[i] = (trial % 4 == 0) ? 1.0 : std::ldexp(static_cast<double>(rng() % 1000 + 1), -10);
		}
		// std: pairs (depth, index), compared by depth only
		std::vector<ValuePair> vals;
		for (int i = 0; i < n; ++i) vals.push_back(ValuePair(depth[i], static_cast<double>(i)));
		std::make_heap(vals.begin(), vals.end(), comparePairFirst);
		std::vector<int> want;
		while (!vals.empty()) {
			std::pop_heap(vals.begin(), vals.end(), comparePairFirst);
			want.push_back(static_cast<int>(vals.back().second));
			vals.pop_back();
		}
		std::vector<uint8_t> heap(n);
		for (int i = 0; i < n; ++i) heap[i] = static_cast<uint8_t>(i);
		auto key = [&](uint8_t t) { return depth[t]; };
		srh::filt::heap_make(heap.data(), 1, n, key);
		std::vector<int> got;
		for (int len = n; len > 0; --len) {
			srh::filt::heap_pop(heap.data(), 1, len, key);
			got.push_back(heap[len - 1]);
		}
		bool same = got == want;
		// the selection loop: the same taps, kept in index order
		std::vector<double> win(121, NaN), wts(121, 0.0);
		for (int i = 0; i < n; ++i) { win[i] = depth[i]; wts[i] = weight[i]; }
		const double ref = fr_weighted_median(win.data(), wts.data(), 5, 0.0, 1e9);
		double total = 0.0;
		for (int i = 0; i < n; ++i) { heap[i] = static_cast<uint8_t>(i); total += weight[i]; }
		const double lib = srh::filt::weighted_median_replay(heap.data(), 1, n, total, key,
		                                                     [&](uint8_t t) { return weight[t]; });
		if (std::memcmp(&ref, &lib, sizeof(double)) != 0) same = false;
		if (!same) ++bad;
	}
	return bad;
}

}  // extern "C"
