// speckle_host.cpp -- csrc/srh_speckle.hpp compiled for the host: its valid / joined / unite / find driven sequentially
// over one map, the way the kernels of srh_speckle.hip drive them in parallel.  Built at test time as a shared library
// (tests/speckle_ref.py, lib()) and loaded with ctypes; with -DSPECKLE_HOST_MAIN it is a program of its own that holds the
// routines against a flood fill on random maps (for a run under -fsanitize=address,undefined on the CPU).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "srh_speckle.hpp"

extern "C" {

// labels[i] = root of pixel i (-1: not valid), sizes[r] = members of the component with label r (0 elsewhere).
// order 0: the joined pairs in pixel order; 1: back to front (the forest must not depend on it)
void sp_label(const uint8_t *mask, const double *D, int w, int h, double max_diff, int order, int32_t *labels, int32_t *sizes)
{
	const int32_t n = w*h;
	std::vector<int32_t> L(n);
	for (int32_t i = 0; i < n; ++i) L[i] = i;
	std::vector<std::pair<int32_t, int32_t> > pairs;
	for (int y = 0; y < h; ++y)
		for (int x = 0; x < w; ++x) {
			const int32_t i = y*w + x;
			if (!srh::cc::valid(mask[i], D[i])) continue;
			if (x + 1 < w && srh::cc::valid(mask[i + 1], D[i + 1]) && srh::cc::joined(D[i], D[i + 1], max_diff)) pairs.push_back(std::make_pair(i, i + 1));
			if (y + 1 < h && srh::cc::valid(mask[i + w], D[i + w]) && srh::cc::joined(D[i], D[i + w], max_diff)) pairs.push_back(std::make_pair(i, i + w));
		}
	for (size_t k = 0; k < pairs.size(); ++k) {
		const std::pair<int32_t, int32_t> &p = pairs[order ? pairs.size() - 1 - k : k];
		if (order) srh::cc::unite(L.data(), p.second, p.first);
		else srh::cc::unite(L.data(), p.first, p.second);
	}
	for (int32_t i = 0; i < n; ++i) sizes[i] = 0;
	for (int32_t i = 0; i < n; ++i) {
		labels[i] = srh::cc::valid(mask[i], D[i]) ? srh::cc::find(L.data(), i) : -1;
		if (labels[i] >= 0) ++sizes[labels[i]];
	}
}

double sp_depth_steps(double min_depth, double max_depth, int levels, double steps)
{
	return srh::cc::depth_steps(min_depth, max_depth, levels, steps);
}

}  // extern "C"

#ifdef SPECKLE_HOST_MAIN
int main()
{
	std::mt19937 rng(20240607u);
	const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();
	int bad = 0;
	for (int trial = 0; trial < 200; ++trial) {
		const int w = 1 + (int)(rng() % 48), h = 1 + (int)(rng() % 40), n = w*h;
		std::vector<uint8_t> mask(n);
		std::vector<double> D(n);
		for (int i = 0; i < n; ++i) {
			mask[i] = rng() % 10 != 0;
			const unsigned k = rng() % 16;
			D[i] = k == 0 ? INF : k == 1 ? NaN : k == 2 ? -1.0 : k == 3 ? -INF : 40.0 + 0.25*(double)(rng() % 4);
		}
		const double max_diff = 0.25*(double)(trial % 3);
		std::vector<int32_t> labels(n), sizes(n), want(n, -1);
		// flood fill in pixel order: a component's first pixel is its smallest index
		for (int s = 0; s < n; ++s) {
			if (want[s] >= 0 || !srh::cc::valid(mask[s], D[s])) continue;
			std::vector<int> stack(1, s);
			want[s] = s;
			while (!stack.empty()) {
				const int i = stack.back(); stack.pop_back();
				const int x = i % w, y = i / w;
				const int nb[4] = { x > 0 ? i - 1 : -1, x + 1 < w ? i + 1 : -1, y > 0 ? i - w : -1, y + 1 < h ? i + w : -1 };
				for (int k = 0; k < 4; ++k) {
					const int j = nb[k];
					if (j < 0 || want[j] >= 0 || !srh::cc::valid(mask[j], D[j]) || !srh::cc::joined(D[i], D[j], max_diff)) continue;
					want[j] = s;
					stack.push_back(j);
				}
			}
		}
		for (int order = 0; order < 2; ++order) {
			sp_label(mask.data(), D.data(), w, h, max_diff, order, labels.data(), sizes.data());
			for (int i = 0; i < n; ++i) if (labels[i] != want[i]) { ++bad; break; }
		}
	}
	std::printf("speckle_host: %d of 400 labellings differ from the flood fill\n", bad);
	return bad ? 1 : 0;
}
#endif
