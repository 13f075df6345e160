// srh_window.hpp -- the support window of one centre pixel (GeodesicWeight / AdaptiveWeight::init_weights), computed by
// one lane into storage the caller chooses: weights_kernel writes it to the band's window buffer, the hole filter
// (srh_filter.hip) to the lane's own LDS.  One body, so both give the same bits (geodesicweight.cpp:59-131,
// adaptiveweight.cpp:33-79).
#pragma once

#include "srh_internal.hpp"
#include "srh_geom.hpp"

namespace srh {

// colour distance between two packed pixels: sqrt(dr*dr + dg*dg + db*db) in double
// (geodesicweight.cpp:89-90, adaptiveweight.cpp:66-68); the squares are small
// integers, so every partial sum is exact.
__device__ __forceinline__ double color_dist(uint32_t a, uint32_t b) {
	const double dr = (double)((int)(a & 255u) - (int)(b & 255u));
	const double dg = (double)((int)((a >> 8) & 255u) - (int)((b >> 8) & 255u));
	const double db = (double)((int)((a >> 16) & 255u) - (int)((b >> 16) & 255u));
	return sqrt(dr*dr + dg*dg + db*db);
}

// The window of (cx, cy) in view V: tap (r, c), r, c in [0, 2R], is the reference's weight(r - R, c - R).
// `wtap(r, c)` returns a reference to that tap's storage.  Taps outside the image keep geodesic_init (geodesic: weight
// exp(-init/sigma)) or get 0 (adaptive).
template <class Tap>
__device__ __forceinline__ void support_window(const ViewDev &V, const srh_params &P, int cx, int cy, Tap wtap)
{
	const int W = V.w, H = V.h;
	const int R = P.window_radius, WS = 2*R + 1;
	if (P.weight_kind == SRH_WEIGHT_GEODESIC) {
		// geodesicweight.cpp:59-131
		for (int i = 0; i < WS*WS; ++i) wtap(i / WS, i % WS) = P.geodesic_init;
		wtap(R, R) = 0.0;
		for (int iter = 0; iter < P.geodesic_iters; ++iter) {
			for (int pass = 0; pass < 2; ++pass) {
				// K1 = (-1,-1)(0,-1)(1,-1)(-1,0) forward; K2 = (-1,1)(0,1)(1,1)(1,0) backward
				const int sy = pass == 0 ? -1 : 1;
				for (int yi = 0; yi < WS; ++yi) {
					const int y = pass == 0 ? (-R + yi) : (R - yi);
					const int py = cy + y;
					for (int xi = 0; xi < WS; ++xi) {
						const int x = pass == 0 ? (-R + xi) : (R - xi);
						const int px = cx + x;
						if (px < 0 || py < 0 || px >= W || py >= H) continue;
						const uint32_t c1 = V.rgba[(size_t)py*W + px];
						double weight = wtap(y + R, x + R);
						for (int k = 0; k < 4; ++k) {
							const int dx = (k == 3) ? (pass == 0 ? -1 : 1) : (k - 1);
							const int dy = (k == 3) ? 0 : sy;
							if (x + dx > R || y + dy > R || x + dx < -R || y + dy < -R) continue;
							const int qx = px + dx, qy = py + dy;
							if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
							const double diff = color_dist(V.rgba[(size_t)qy*W + qx], c1);
							const double cost = wtap(y + dy + R, x + dx + R);
							const double cand = cost + diff;
							if (cand < weight) weight = cand;
						}
						wtap(y + R, x + R) = weight;
					}
				}
			}
		}
		for (int i = 0; i < WS*WS; ++i) wtap(i / WS, i % WS) = exp(-wtap(i / WS, i % WS) / P.geodesic_sigma);
	} else {
		// adaptiveweight.cpp:33-79 (the centre pixel is always in bounds here)
		const uint32_t crgb = V.rgba[(size_t)cy*W + cx];
		for (int row = -R; row <= R; ++row) {
			const double dwr = exp(-abs(row) / (1.0*R));
			for (int col = -R; col <= R; ++col) {
				double weight = 0.0;
				const int px = cx + col, py = cy + row;
				if (!(px < 0 || py < 0 || px >= W || py >= H)) {
					const double diff = color_dist(V.rgba[(size_t)py*W + px], crgb);
					const double w1 = dwr*exp(-abs(col) / (1.0*R));
					const double w2 = exp(-diff / P.adaptive_color_sigma);
					weight = w1*w2;
					if (isnan_d(weight)) weight = 0.0;
				}
				wtap(row + R, col + R) = weight;
			}
		}
	}
}

}  // namespace srh
