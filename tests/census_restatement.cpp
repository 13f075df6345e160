// census_restatement.cpp -- CPU restatement of the support-weighted census cost (option "cost" = SRH_COST_CENSUS;
// DESIGN.md 4p) and of one WTA pass of computeCostVolumes (stereo/twoviewstereo.cpp:260-333) with it.  The cost is not in
// the reference: it keeps cost_sad's tap rule (:864-905) and replaces the per-tap term by the Hamming distance of two 9x7
// census signatures, accumulated with one fused multiply-add.  The census tests (tests/test_census_host.py,
// tests/test_gpu_census.py) hold the library against it.  Built with g++ -ffp-contract=off at test time
// (tests/census_ref.py) and linked to the oracle: sro_weights, sro_unproject, sro_epipolar_curve, sro_closest_points.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

extern "C" {
#include "sr_oracle.h"
}

namespace {

// mask.pixel(x, y) == WHITE (out of bounds: not WHITE)
bool white(const sro_image *img, int x, int y) {
	if (x < 0 || y < 0 || x >= img->w || y >= img->h) return false;
	return !img->mask || img->mask[(size_t)y*img->w + x] == 1;
}

// the `gray` plane: toGray of every pixel of the image, whatever the mask says
double pixel_gray(const sro_image *img, int x, int y) {
	const uint8_t *px = img->rgba + 4*((size_t)y*img->w + x);
	return sro_to_gray((double)px[0], (double)px[1], (double)px[2]);
}

// the left tap counts where left.sample() is valid behind leftMask: inside, x + 1 < w, y + 1 < h, mask WHITE
bool left_counts(const sro_image *img, int x, int y) {
	return white(img, x, y) && x + 1 < img->w && y + 1 < img->h;
}

// twoviewstereo.cpp:287-300: depth of the mid-point of closest approach, in the reference camera
double candidate_depth(const sro_camera *refcam, const sro_camera *othcam, const sro_params *p,
                       const double rsrc[3], const double rdir[3], int cx, int cy)
{
	double s2[3], d2[3], p1[3], p2[3];
	sro_unproject(othcam, (cx + 0.5) / p->image_scale, (cy + 0.5) / p->image_scale, s2, d2);
	sro_closest_points(rsrc, rdir, s2, d2, p1, p2);
	p1[0] += p2[0]; p1[1] += p2[1]; p1[2] += p2[2];
	p1[0] *= 0.5;   p1[1] *= 0.5;   p1[2] *= 0.5;
	return ((refcam->R[6]*p1[0] + refcam->R[7]*p1[1]) + refcam->R[8]*p1[2]) + refcam->t[2];
}

int popcount64(uint64_t v) { return __builtin_popcountll(v); }

}  // namespace

extern "C" {

// the signature of pixel (x, y): bit (dy + 3)*9 + (dx + 4) for dy in -3..3, dx in -4..4, set iff the neighbour is not the
// centre, lies inside the image and is darker than the centre
uint64_t sr_census_signature(const sro_image *img, int x, int y)
{
	const double centre = pixel_gray(img, x, y);
	uint64_t sig = 0;
	for (int dy = -3; dy <= 3; ++dy) {
		for (int dx = -4; dx <= 4; ++dx) {
			if (dx == 0 && dy == 0) continue;
			const int nx = x + dx, ny = y + dy;
			if (nx < 0 || ny < 0 || nx >= img->w || ny >= img->h) continue;
			if (pixel_gray(img, nx, ny) < centre) sig |= (uint64_t)1 << ((dy + 3)*9 + (dx + 4));
		}
	}
	return sig;
}

// the signature plane, w*h words
void sr_census_plane(const sro_image *img, uint64_t *out)
{
	for (int y = 0; y < img->h; ++y)
		for (int x = 0; x < img->w; ++x) out[(size_t)y*img->w + x] = sr_census_signature(img, x, y);
}

// the cost with the window of (x1, y1): weights[(row + R)*(2R + 1) + (col + R)]; sl / sr: the two signature planes
double sr_cost_census(const sro_image *left, const sro_image *right, const uint64_t *sl, const uint64_t *sr,
                      const double *weights, const sro_params *p, int x1, int y1, int x2, int y2)
{
	const int R = p->window_radius, WS = 2*R + 1;
	int numPixels = 0;
	double sum = 0.0, totalWeight = 0.0;
	for (int row = -R; row <= R; ++row) {
		for (int col = -R; col <= R; ++col) {
			if (!left_counts(left, x1 + col, y1 + row)) continue;
			if (!white(right, x2 + col, y2 + row)) continue;
			const double weight = weights[(row + R)*WS + (col + R)];
			if (weight > p->weight_cutoff) {
				const int h = popcount64(sl[(size_t)(y1 + row)*left->w + (x1 + col)] ^ sr[(size_t)(y2 + row)*right->w + (x2 + col)]);
				sum = std::fma(weight, (double)h, sum);
				totalWeight += weight;
				++numPixels;
			}
		}
	}
	if (numPixels <= 4 || totalWeight <= 1e-10) return p->bad_ret;
	return sum / totalWeight;
}

// the cost of n pairs xy[4k..4k+3], each with the window of its own (x1, y1) (sro_weights)
void sr_pair_costs_census(const sro_image *left, const sro_image *right, const sro_params *p, int n, const int32_t *xy,
                          double *out)
{
	const int WS = 2*p->window_radius + 1;
	std::vector<double> weights((size_t)WS*WS);
	std::vector<uint64_t> sl((size_t)left->w*left->h), sr((size_t)right->w*right->h);
	sr_census_plane(left, sl.data());
	sr_census_plane(right, sr.data());
	for (int k = 0; k < n; ++k) {
		sro_weights(left, xy[4*k], xy[4*k + 1], p, weights.data());
		out[k] = sr_cost_census(left, right, sl.data(), sr.data(), weights.data(), p, xy[4*k], xy[4*k + 1], xy[4*k + 2], xy[4*k + 3]);
	}
}

// one pass of computeCostVolumes with the census cost, rows [y0, y1) of `depth` (w*h) written; min_cost (optional) the
// WTA's; win_xy (optional, 2 per pixel): the winning candidate, (-1, -1) = none
void sr_twoview_wta_census(const sro_image *ref, const sro_image *oth, const sro_camera *refcam, const sro_camera *othcam,
                           const sro_params *p, int y0, int y1, double *depth, double *min_cost, int32_t *win_xy)
{
	const int W = ref->w, WS = 2*p->window_radius + 1;
	std::vector<double> weights((size_t)WS*WS);
	std::vector<int32_t> curve(2*4096);
	std::vector<uint64_t> sl((size_t)ref->w*ref->h), sr((size_t)oth->w*oth->h);
	sr_census_plane(ref, sl.data());
	sr_census_plane(oth, sr.data());
	for (int y = y0; y < y1; ++y) {
		for (int x = 0; x < W; ++x) {
			const size_t pv = (size_t)y*W + x;
			depth[pv] = NAN;
			if (min_cost) min_cost[pv] = INFINITY;
			if (win_xy) win_xy[2*pv] = win_xy[2*pv + 1] = -1;
			if (!white(ref, x, y)) continue;
			sro_weights(ref, x, y, p, weights.data());
			double rsrc[3], rdir[3];
			sro_unproject(refcam, (x + 0.5) / p->image_scale, (y + 0.5) / p->image_scale, rsrc, rdir);
			int n = sro_epipolar_curve(refcam, othcam, oth, p, 0, x, y, curve.data(), (int)(curve.size()/2));
			if (n > (int)(curve.size()/2)) {
				curve.resize(2*(size_t)n);
				n = sro_epipolar_curve(refcam, othcam, oth, p, 0, x, y, curve.data(), n);
			}
			double secondBestCost = INFINITY, minCost = INFINITY;
			for (int i = 0; i < n; ++i) {
				const int cx = curve[2*i], cy = curve[2*i + 1];
				const double cost = sr_cost_census(ref, oth, sl.data(), sr.data(), weights.data(), p, x, y, cx, cy);
				if (cost + p->wta_margin < minCost) {
					secondBestCost = minCost;
					minCost = cost;
					depth[pv] = candidate_depth(refcam, othcam, p, rsrc, rdir, cx, cy);
					if (win_xy) { win_xy[2*pv] = cx; win_xy[2*pv + 1] = cy; }
				}
			}
			if (minCost > p->second_best_factor*secondBestCost)
				depth[pv] = INFINITY;
			if (min_cost) min_cost[pv] = minCost;
		}
	}
}

}  // extern "C"
