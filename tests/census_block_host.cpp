// census_block_host.cpp -- the library's srh_census_block.hpp (stereoreconstruction_amd/csrc: the per-tile settle of the
// reference side, the fast-form and select-form block sums and the finish of the census cost on the dense plan) compiled
// for the host and held, bit for bit, to sr_cost_census of tests/census_restatement.cpp -- including which candidates are
// bad_ret.
// A program of its own (tests/test_census_block_host.py builds it with g++ -O1 -ffp-contract=off, once more with
// -fsanitize=address,undefined, and runs both): usage  census_block_host <pair file> <radius 2|5>, exit status 0 = every
// check held.  Pair file: int32 w, h; rgba of the left and the right view (w*h*4 bytes each); their masks (w*h bytes each).
//
// Every pixel of the left view against every column of its row in the right view, in blocks of 8 adjacent columns from even
// starts as the kernel cuts them: the select form for every candidate, the fast form (8 and 2 candidates wide) for every
// candidate whose window in the right view is fully usable.  Weights from the oracle, geodesic and adaptive, under three
// cut-offs: the default, one that equals a weight of the pair's centre window (taps at and below it are skipped), and a
// negative one (a counting tap may weigh 0.0).  The row source is a plain-array one: pointers into planes with a border of
// CENSUS_UNUSABLE words, the other view's rows 16-byte aligned at even columns as the kernel's rings are.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "srh_census_block.hpp"

extern "C" {
#include "sr_oracle.h"
void sr_census_plane(const sro_image *img, uint64_t *out);
double sr_cost_census(const sro_image *left, const sro_image *right, const uint64_t *sl, const uint64_t *sr,
                      const double *weights, const sro_params *p, int x1, int y1, int x2, int y2);
}

namespace {

const int NCB = 8;
const int PADY = 8;                 // rows of border: radius 5 + slack

long n_checked = 0, n_failed = 0;

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void expect(bool ok, const char *what, int R, int x, int y, int c, double got, double want) {
	++n_checked;
	if (ok) return;
	if (++n_failed <= 20) std::fprintf(stderr, "FAIL %s: r=%d pixel (%d, %d) column %d: got %.17g want %.17g\n", what, R, x, y, c, got, want);
}

bool white(const sro_image &img, int x, int y) {
	return x >= 0 && y >= 0 && x < img.w && y < img.h && (!img.mask || img.mask[(size_t)y*img.w + x] == 1);
}

// A view's signatures with a border of CENSUS_UNUSABLE: column x of row y at at(x, y); column -R sits on an even index of a
// 16-byte aligned row, so a block's segment from an even candidate column is aligned as in the kernel's ring.
// reference side: unusable where left.sample() is (outside, last column, last row, behind the mask); other side: unusable
// outside and behind the mask.
struct Plane {
	int padl, stride;
	std::vector<uint64_t> store;
	uint64_t *base;
	Plane(const sro_image &img, const std::vector<uint64_t> &sig, int R, bool reference_side)
		: padl(R + 16), stride((img.w + 2*(R + 16) + 1) & ~1), store((size_t)stride*(img.h + 2*PADY) + 2, srh::CENSUS_UNUSABLE)
	{
		base = store.data() + (((uintptr_t)store.data() & 15) ? 1 : 0);
		for (size_t k = 0; k < (size_t)stride*(img.h + 2*PADY); ++k) base[k] = srh::CENSUS_UNUSABLE;
		for (int y = 0; y < img.h; ++y)
			for (int x = 0; x < img.w; ++x) {
				const bool ok = white(img, x, y) && (!reference_side || (x + 1 < img.w && y + 1 < img.h));
				if (ok) base[(size_t)(y + PADY)*stride + x + padl] = sig[(size_t)y*img.w + x];
			}
	}
	const uint64_t *at(int x, int y) const { return base + (size_t)(y + PADY)*stride + x + padl; }
};

// the row source: the window of (x, y) against the block whose first candidate is column c0 of the same row
template <int R>
struct ArrayRows {
	static constexpr int WS = 2*R + 1, WP = (WS + 1) & ~1;
	const Plane *L, *O;
	const double *w;                    // [WS][WP], settled
	const unsigned *okm;                // [WS]
	int x, y, c0;
	srh::CensusRow row(int row) const {
		return srh::CensusRow{ O->at(c0 - R, y - R + row), w + row*WP, L->at(x - R, y - R + row), okm[row] };
	}
};

struct Tally { long fast = 0, select_only = 0, bad = 0, skipped_weights = 0, zero_weight_counts = 0; };

template <int R>
void run(const sro_image &left, const sro_image &right, const std::vector<uint64_t> &sl, const std::vector<uint64_t> &sr,
         sro_params p, Tally &t)
{
	constexpr int WS = 2*R + 1, WP = (WS + 1) & ~1;
	p.window_radius = R;
	const Plane L(left, sl, R, true), O(right, sr, R, false);
	const int W = left.w, H = left.h, OW = right.w;
	std::vector<double> weights(WS*WS);
	std::vector<char> full(OW);
	for (int y = 0; y < H; ++y) {
		for (int c = 0; c < OW; ++c) {
			bool ok = true;
			for (int row = -R; row <= R; ++row)
				for (int col = -R; col <= R; ++col) ok = ok && white(right, c + col, y + row);
			full[c] = ok;
		}
		for (int x = 0; x < W; ++x) {
			sro_weights(&left, x, y, &p, weights.data());
			double w[WS*WP];
			unsigned okm[WS];
			for (int row = 0; row < WS; ++row) {
				for (int col = 0; col < WP; ++col) w[row*WP + col] = col < WS ? weights[row*WS + col] : 0.0;
				okm[row] = srh::census_settle_row<WS>(L.at(x - R, y - R + row), w + row*WP, p.weight_cutoff);
				for (int col = 0; col < WS; ++col) {
					const bool counts = (okm[row] >> col) & 1u;
					if (!counts && srh::census_usable(L.at(x - R, y - R + row)[col])) ++t.skipped_weights;   // (skipped for its weight alone)
					if (counts && weights[row*WS + col] == 0.0) ++t.zero_weight_counts;
					// a skipped tap's weight is +0.0, a counting tap keeps its own
					const double want = counts ? weights[row*WS + col] : 0.0;
					expect(same_bits(w[row*WP + col], want), "settled weight", R, x, y, row*WS + col, w[row*WP + col], want);
				}
			}
			double tw;
			int npx;
			srh::census_pixel_totals<WS>(ArrayRows<R>{ &L, &O, w, okm, x, y, 0 }, tw, npx);
			for (int c0 = 0; c0 < OW; c0 += NCB) {
				const ArrayRows<R> src{ &L, &O, w, okm, x, y, c0 };
				double s[NCB], tt[NCB], acc8[NCB], acc2[2];
				int np[NCB];
				srh::census_select_block<WS, NCB>(src, s, tt, np);
				srh::census_fast_block<WS, NCB>(src, acc8);
				srh::census_fast_block<WS, 2>(src, acc2);
				for (int j = 0; j < NCB && c0 + j < OW; ++j) {
					const int c = c0 + j;
					const double want = sr_cost_census(&left, &right, sl.data(), sr.data(), weights.data(), &p, x, y, c, y);
					if (want == p.bad_ret) ++t.bad;
					const double sel = srh::census_finish(np[j], tt[j], s[j], p.bad_ret);
					expect(same_bits(sel, want), "select form", R, x, y, c, sel, want);
					if (!full[c]) { ++t.select_only; continue; }
					++t.fast;
					const double f8 = srh::census_finish(npx, tw, acc8[j], p.bad_ret);
					expect(same_bits(f8, want), "fast form, 8 wide", R, x, y, c, f8, want);
					if (j < 2) {
						const double f2 = srh::census_finish(npx, tw, acc2[j], p.bad_ret);
						expect(same_bits(f2, want), "fast form, 2 wide", R, x, y, c, f2, want);
					}
				}
			}
		}
	}
}

std::vector<uint8_t> slurp(FILE *f, size_t n) {
	std::vector<uint8_t> v(n);
	if (std::fread(v.data(), 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
	return v;
}

}  // namespace

int main(int argc, char **argv)
{
	if (argc < 3) { std::fprintf(stderr, "usage: %s <pair file> <radius 2|5>\n", argv[0]); return 2; }
	FILE *f = std::fopen(argv[1], "rb");
	if (!f) { std::perror(argv[1]); return 2; }
	int32_t wh[2];
	if (std::fread(wh, sizeof(int32_t), 2, f) != 2) { std::fprintf(stderr, "short read\n"); return 2; }
	const int w = wh[0], h = wh[1], R = std::atoi(argv[2]);
	const size_t n = (size_t)w*h;
	const std::vector<uint8_t> lrgba = slurp(f, 4*n), rrgba = slurp(f, 4*n), lmask = slurp(f, n), rmask = slurp(f, n);
	std::fclose(f);
	const sro_image left = { w, h, lrgba.data(), lmask.data() }, right = { w, h, rrgba.data(), rmask.data() };
	std::vector<uint64_t> sl(n), sr(n);
	sr_census_plane(&left, sl.data());
	sr_census_plane(&right, sr.data());

	for (int kind = 0; kind < 2; ++kind) {
		sro_params p;
		sro_params_twoview_defaults(&p);
		p.weight_kind = kind == 0 ? SRO_WEIGHT_GEODESIC : SRO_WEIGHT_ADAPTIVE;
		p.window_radius = R;
		// a weight of the centre pixel's window, off its centre: taps that weigh exactly this much are at the cut-off, skipped
		std::vector<double> wc((2*R + 1)*(2*R + 1));
		sro_weights(&left, w/2, h/2, &p, wc.data());
		const double cutoffs[3] = { p.weight_cutoff, wc[(2*R + 1) + 1], -1.0 };
		for (int k = 0; k < 3; ++k) {
			p.weight_cutoff = cutoffs[k];
			Tally t;
			if (R == 5) run<5>(left, right, sl, sr, p, t);
			else if (R == 2) run<2>(left, right, sl, sr, p, t);
			else { std::fprintf(stderr, "radius 2 or 5\n"); return 2; }
			std::printf("r=%d %s cut-off %.3g: %ld fast, %ld select-only candidates, %ld bad_ret, %ld weights skipped, %ld counting taps of weight 0\n",
			            R, kind == 0 ? "geodesic" : "adaptive", cutoffs[k], t.fast, t.select_only, t.bad, t.skipped_weights, t.zero_weight_counts);
			// the run must have met what it is about
			if (t.fast == 0 || t.select_only == 0 || t.bad == 0) { std::fprintf(stderr, "FAIL: a form or bad_ret never met\n"); ++n_failed; }
			if (k == 1 && t.skipped_weights == 0) { std::fprintf(stderr, "FAIL: no weight at or below the raised cut-off\n"); ++n_failed; }
		}
	}
	std::printf("%ld checked, %ld failed\n", n_checked, n_failed);
	return n_failed == 0 ? 0 : 1;
}
