// sad_restatement.cpp -- CPU restatement of TwoViewStereo::cost_sad (stereo/twoviewstereo.cpp:864-905) and of one pass
// of computeCostVolumes with it (:260-333, the cost_ncc call replaced by cost_sad), written as the reference's loops are.
// The SAD tests (tests/test_sad_host.py, tests/test_gpu_sad.py) hold the library against it.  Built with g++
// -ffp-contract=off at test time (tests/sad_ref.py) and linked to the oracle: sro_weights, sro_unproject,
// sro_epipolar_curve, sro_closest_points.
#include <cmath>
#include <cstdlib>
#include <vector>

extern "C" {
#include "sr_oracle.h"
}

namespace {

// leftMask.pixel(x, y) == WHITE (out of bounds: not WHITE)
bool white(const sro_image *img, int x, int y) {
	if (x < 0 || y < 0 || x >= img->w || y >= img->h) return false;
	return !img->mask || img->mask[(size_t)y*img->w + x] == 1;
}

// left.sample(x, y) at integer coordinates (vectorimage.cpp:129-155), toGray
bool sample_gray(const sro_image *img, int x, int y, double *g) {
	double rgb[3];
	if (!sro_image_sample(img, (double)x, (double)y, rgb)) return false;
	*g = sro_to_gray(rgb[0], rgb[1], rgb[2]);
	return true;
}

// right.pixel(x, y): every pixel of the image is valid (VectorImage::fromQImage), toGray
bool pixel_gray(const sro_image *img, int x, int y, double *g) {
	if (x < 0 || y < 0 || x >= img->w || y >= img->h) return false;
	const uint8_t *px = img->rgba + 4*((size_t)y*img->w + x);
	*g = sro_to_gray((double)px[0], (double)px[1], (double)px[2]);
	return true;
}

// twoviewstereo.cpp:287-300: depth of the mid-point of closest approach, in the reference camera (static in sr_oracle.c)
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

}  // namespace

extern "C" {

// cost_sad with the window of (x1, y1): weights[(row + R)*(2R + 1) + (col + R)] = weightFuncs(row, col)
double sr_cost_sad(const sro_image *left, const sro_image *right, const double *weights, const sro_params *p,
                   int x1, int y1, int x2, int y2)
{
	const int R = p->window_radius, WS = 2*R + 1;
	int numPixels = 0;
	double sum = 0.0, totalWeight = 0.0;
	for (int row = -R; row <= R; ++row) {
		for (int col = -R; col <= R; ++col) {
			if (!white(left, x1 + col, y1 + row)) continue;
			if (!white(right, x2 + col, y2 + row)) continue;
			double gl, gr;
			if (!sample_gray(left, x1 + col, y1 + row, &gl)) continue;
			if (!pixel_gray(right, x2 + col, y2 + row, &gr)) continue;
			const double weight = weights[(row + R)*WS + (col + R)];
			if (weight > p->weight_cutoff) {
				const double diff = fabs(gl - gr);
				const double MAX_COLOR_DIFF = p->max_color_diff;
				sum += weight*((diff < MAX_COLOR_DIFF) ? diff : MAX_COLOR_DIFF);   // min(MAX_COLOR_DIFF, diff)
				totalWeight += weight;
				++numPixels;
			}
		}
	}
	if (numPixels <= 4 || totalWeight <= 1e-10) return p->bad_ret;
	return (sum / totalWeight);
}

// cost_sad of n pairs xy[4k..4k+3], each with the window of its own (x1, y1) (sro_weights)
void sr_pair_costs_sad(const sro_image *left, const sro_image *right, const sro_params *p, int n, const int32_t *xy,
                       double *out)
{
	const int WS = 2*p->window_radius + 1;
	std::vector<double> weights((size_t)WS*WS);
	for (int k = 0; k < n; ++k) {
		sro_weights(left, xy[4*k], xy[4*k + 1], p, weights.data());
		out[k] = sr_cost_sad(left, right, weights.data(), p, xy[4*k], xy[4*k + 1], xy[4*k + 2], xy[4*k + 3]);
	}
}

// one pass of computeCostVolumes with cost_sad, rows [y0, y1) of `depth` (w*h) written; min_cost (optional) the WTA's
void sr_twoview_wta_sad(const sro_image *ref, const sro_image *oth, const sro_camera *refcam, const sro_camera *othcam,
                        const sro_params *p, int y0, int y1, double *depth, double *min_cost)
{
	const int W = ref->w, WS = 2*p->window_radius + 1;
	std::vector<double> weights((size_t)WS*WS);
	std::vector<int32_t> curve(2*4096);
	for (int y = y0; y < y1; ++y) {
		for (int x = 0; x < W; ++x) {
			const size_t pv = (size_t)y*W + x;
			depth[pv] = NAN;
			if (min_cost) min_cost[pv] = INFINITY;
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
				const double cost = sr_cost_sad(ref, oth, weights.data(), p, x, y, cx, cy);
				if (cost + p->wta_margin < minCost) {
					secondBestCost = minCost;
					minCost = cost;
					depth[pv] = candidate_depth(refcam, othcam, p, rsrc, rdir, cx, cy);
				}
			}
			if (minCost > p->second_best_factor*secondBestCost)
				depth[pv] = INFINITY;
			if (min_cost) min_cost[pv] = minCost;
		}
	}
}

}  // extern "C"
