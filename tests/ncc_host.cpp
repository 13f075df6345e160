// ncc_host.cpp -- the library's srh_ncc.hpp (stereoreconstruction_amd/csrc) compiled for the host and held to the oracle,
// bit for bit: ncc_select_cost against sro_twoview_cost_ncc, pixel_constants against pix_const of f32_restatement.cpp.
// A program of its own (tests/test_ncc_host.py builds it with g++ -O1 -ffp-contract=off, once more with
// -fsanitize=address,undefined, and runs both): usage  ncc_host <pair file>, exit status 0 = every check held.
// Pair file: int32 w, h; rgba of the left and the right view (w*h*4 bytes each); their masks (w*h bytes each, 1 = in).
//
// Every reference pixel of the left view against every column of its row in the right view, five columns outside each
// side included, at radius 2 and 5, with geodesic and adaptive weights, and once with a cut-off that removes taps.
// The taps reach ncc_select_cost in the two ways the kernels use: through pointers and strides into NaN-bordered planes
// (window_exact_cost of srh_walk.hpp) and through rings of WS + 1 row slots that wrap (strip_cost_general of
// srh_strip.hip).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "srh_ncc.hpp"

extern "C" {
#include "sr_oracle.h"
void f32r_gray_plane(const sro_image *img, double *out);
int f32r_pix_const(const double *w, const double *l, int T, double cutoff, double c[4]);
}

namespace {

const int PAD = 16;                 // NaN border of the padded planes: radius 5 + five columns outside + slack
const int OUTSIDE = 5;

long n_checked = 0, n_failed = 0;

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

void expect(bool ok, const char *what, int R, int x, int y, int c, double got, double want) {
	++n_checked;
	if (ok) return;
	if (++n_failed <= 20) std::fprintf(stderr, "FAIL %s: r=%d pixel (%d, %d) column %d: got %.17g want %.17g\n", what, R, x, y, c, got, want);
}

struct Padded {
	int w, h, stride;
	std::vector<double> v;
	Padded(const sro_image &img) : w(img.w), h(img.h), stride(img.w + 2*PAD), v((size_t)(img.w + 2*PAD)*(img.h + 2*PAD), NAN) {
		std::vector<double> g((size_t)w*h);
		f32r_gray_plane(&img, g.data());
		for (int y = 0; y < h; ++y)
			for (int x = 0; x < w; ++x) v[(size_t)(y + PAD)*stride + (x + PAD)] = g[(size_t)y*w + x];
	}
	const double *at(int x, int y) const { return &v[(size_t)(y + PAD)*stride + (x + PAD)]; }
};

struct Tally { long windows = 0, all_true = 0, cut_taps = 0, kept_taps = 0, bad_ret = 0, clamped = 0, ranged = 0; };

template <int R>
void run(const sro_image &left, const sro_image &right, const Padded &L, const Padded &Rp, sro_params p, Tally &t)
{
	constexpr int WS = 2*R + 1, T = WS*WS, NS = WS + 1;
	p.window_radius = R;
	const int W = left.w, H = left.h, SP = L.stride;
	std::vector<double> w(T), l(T);
	std::vector<double> ringl((size_t)NS*SP), ringr((size_t)NS*SP);
	for (int y = 0; y < H; ++y) {
		// the rings: window row `row` of image row y in slot (s0 + row) mod NS, whole padded rows
		const int s0 = y % NS;
		for (int row = 0; row < WS; ++row) {
			const int sl = (s0 + row) % NS;
			std::memcpy(&ringl[(size_t)sl*SP], L.at(-PAD, y - R + row), sizeof(double)*SP);
			std::memcpy(&ringr[(size_t)sl*SP], Rp.at(-PAD, y - R + row), sizeof(double)*SP);
		}
		for (int x = 0; x < W; ++x) {
			sro_weights(&left, x, y, &p, w.data());
			const double *lp = L.at(x - R, y - R);
			bool usable = true;
			double sum_wl = 0, sum_w = 0;
			for (int row = 0; row < WS; ++row)
				for (int col = 0; col < WS; ++col) {
					const double gl = lp[(size_t)row*SP + col], wt = w[row*WS + col];
					l[row*WS + col] = gl;
					usable = usable && gl == gl && wt > p.weight_cutoff;
					if (wt > p.weight_cutoff) ++t.kept_taps; else ++t.cut_taps;
					sum_wl += wt*gl;
					sum_w += wt;
				}
			++t.windows;

			// ---- pixel_constants against pix_const
			auto rows_l = [&](int row, double *gl, double *wt) {
				for (int col = 0; col < WS; ++col) { gl[col] = lp[(size_t)row*SP + col]; wt[col] = w[row*WS + col]; }
			};
			double pc[4];
			const bool pall = f32r_pix_const(w.data(), l.data(), T, p.weight_cutoff, pc) != 0;
			const srh::PixelConstants c = srh::pixel_constants<WS, true>(rows_l, p.weight_cutoff, true);
			expect(same_bits(c.mL, pc[0]), "pixel_constants mL", R, x, y, -1, c.mL, pc[0]);
			expect(same_bits(c.tw, pc[1]), "pixel_constants tw", R, x, y, -1, c.tw, pc[1]);
			expect(same_bits(c.s2, pc[2]), "pixel_constants s2", R, x, y, -1, c.s2, pc[2]);
			expect(same_bits(c.sa, pc[3]), "pixel_constants sa", R, x, y, -1, c.sa, pc[3]);
			expect(c.all == pall, "pixel_constants all against pix_const", R, x, y, -1, c.all, pall);
			expect(c.all == (usable && !(sum_w < 1e-10)), "all = every tap usable", R, x, y, -1, c.all, usable);
			if (c.all) ++t.all_true;
			// without SA: the same, sa left at 0
			const srh::PixelConstants c0 = srh::pixel_constants<WS, false>(rows_l, p.weight_cutoff, true);
			expect(same_bits(c0.mL, c.mL) && same_bits(c0.tw, c.tw) && same_bits(c0.s2, c.s2) && c0.all == c.all && same_bits(c0.sa, 0.0),
			       "pixel_constants without SA", R, x, y, -1, c0.s2, c.s2);
			// a false seed: the undivided sum, s2 = 0
			const srh::PixelConstants cf = srh::pixel_constants<WS, true>(rows_l, p.weight_cutoff, false);
			expect(!cf.all && same_bits(cf.mL, sum_wl) && same_bits(cf.tw, sum_w) && same_bits(cf.s2, 0.0) && same_bits(cf.sa, 0.0),
			       "false seed", R, x, y, -1, cf.mL, sum_wl);
			// the row-range form over the window rows on image rows with taps at all (rows 0 .. H - 2, as the strip kernel's
			// border tiles take them): every other row of such a window is unusable, and the constants are those of the
			// window made of rows [ra, rb) alone
			const int ra = y < R ? R - y : 0, rb = y + R > H - 2 ? WS - (y + R - (H - 2)) : WS;
			if (ra < rb) {
				bool others_unusable = true;
				for (int row = 0; row < WS; ++row)
					if (row < ra || row >= rb)
						for (int col = 0; col < WS; ++col) others_unusable = others_unusable && !(l[row*WS + col] == l[row*WS + col]);
				expect(others_unusable, "rows outside [ra, rb) unusable", R, x, y, -1, ra, rb);
				const bool rall = f32r_pix_const(w.data() + ra*WS, l.data() + ra*WS, (rb - ra)*WS, p.weight_cutoff, pc) != 0;
				const srh::PixelConstants cr = srh::pixel_constants<WS, true>(rows_l, p.weight_cutoff, true, ra, rb);
				expect(same_bits(cr.mL, pc[0]) && same_bits(cr.tw, pc[1]) && same_bits(cr.s2, pc[2]) && same_bits(cr.sa, pc[3]) && cr.all == rall,
				       "row-range form", R, x, y, -1, cr.s2, pc[2]);
				if (ra > 0 || rb < WS) ++t.ranged;
				else expect(same_bits(cr.mL, c.mL) && same_bits(cr.s2, c.s2) && cr.all == c.all, "range [0, WS) = default", R, x, y, -1, cr.s2, c.s2);
			}

			// ---- ncc_select_cost against the oracle, both ways
			for (int cx = -OUTSIDE; cx < right.w + OUTSIDE; ++cx) {
				const double want = sro_twoview_cost_ncc(&left, &right, w.data(), &p, x, y, cx, y);
				const double *rp = Rp.at(cx - R, y - R);
				const double *wq = w.data();
				const int wrow = WS, wcol = 1, SPR = Rp.stride;
				const double by_ptr = srh::ncc_select_cost<WS>([&](int row, double *gl, double *gr, double *wt) {
					for (int col = 0; col < WS; ++col) { gl[col] = lp[(size_t)row*SP + col]; gr[col] = rp[(size_t)row*SPR + col]; wt[col] = wq[row*wrow + col*wcol]; }
				}, p.weight_cutoff, p.bad_ret, p.max_color_diff);
				const int i = x - R + PAD, rc = cx - R + PAD;
				const double by_ring = srh::ncc_select_cost<WS>([&](int row, double *gl, double *gr, double *wt) {
					const int sl = s0 + row >= NS ? s0 + row - NS : s0 + row;
					for (int col = 0; col < WS; ++col) { gl[col] = ringl[(size_t)sl*SP + i + col]; gr[col] = ringr[(size_t)sl*SP + rc + col]; wt[col] = w[row*WS + col]; }
				}, p.weight_cutoff, p.bad_ret, p.max_color_diff);
				expect(same_bits(by_ptr, want), "ncc_select_cost, pointers", R, x, y, cx, by_ptr, want);
				expect(same_bits(by_ring, want), "ncc_select_cost, ring", R, x, y, cx, by_ring, want);
				if (want == p.bad_ret) ++t.bad_ret;
				if (want == p.max_color_diff) ++t.clamped;
			}
		}
	}
}

}  // namespace

int main(int argc, char **argv)
{
	if (argc != 2) { std::fprintf(stderr, "usage: ncc_host <pair file>\n"); return 2; }
	FILE *f = std::fopen(argv[1], "rb");
	if (!f) { std::perror(argv[1]); return 2; }
	int32_t wh[2];
	if (std::fread(wh, sizeof wh, 1, f) != 1 || wh[0] <= 0 || wh[1] <= 0 || wh[0] > 4096 || wh[1] > 4096) { std::fclose(f); return 2; }
	const size_t n = (size_t)wh[0]*wh[1];
	std::vector<uint8_t> rgba[2] = { std::vector<uint8_t>(4*n), std::vector<uint8_t>(4*n) }, mask[2] = { std::vector<uint8_t>(n), std::vector<uint8_t>(n) };
	bool ok = std::fread(rgba[0].data(), 1, 4*n, f) == 4*n && std::fread(rgba[1].data(), 1, 4*n, f) == 4*n
	       && std::fread(mask[0].data(), 1, n, f) == n && std::fread(mask[1].data(), 1, n, f) == n;
	std::fclose(f);
	if (!ok) { std::fprintf(stderr, "%s: short file\n", argv[1]); return 2; }
	const sro_image left = { wh[0], wh[1], rgba[0].data(), mask[0].data() }, right = { wh[0], wh[1], rgba[1].data(), mask[1].data() };
	const Padded L(left), Rp(right);

	Tally plain, cut;
	for (int kind = 0; kind < 2; ++kind) {
		sro_params p;
		sro_params_twoview_defaults(&p);
		p.weight_kind = kind == 0 ? SRO_WEIGHT_GEODESIC : SRO_WEIGHT_ADAPTIVE;
		run<2>(left, right, L, Rp, p, plain);
		run<5>(left, right, L, Rp, p, plain);
	}
	{
		// a cut-off that removes taps: geodesic weights are exp(-distance/sigma), 1 at the centre
		sro_params p;
		sro_params_twoview_defaults(&p);
		p.weight_kind = SRO_WEIGHT_GEODESIC;
		p.weight_cutoff = 0.5;
		run<2>(left, right, L, Rp, p, cut);
	}
	std::printf("%dx%d: %ld checks, %ld failed; %ld windows (%ld with every tap usable, %ld over a row range), %ld costs at bad_ret, %ld clamped; "
	            "cut-off case: %ld taps cut, %ld kept, %ld windows with every tap usable\n", wh[0], wh[1], n_checked, n_failed,
	            plain.windows, plain.all_true, plain.ranged, plain.bad_ret + cut.bad_ret, plain.clamped + cut.clamped,
	            cut.cut_taps, cut.kept_taps, cut.all_true);
	// the cases must have met what they are there for
	if (plain.ranged == 0 || plain.bad_ret == 0 || cut.cut_taps == 0 || cut.kept_taps == 0) { std::fprintf(stderr, "a case met none of its windows\n"); return 1; }
	return n_failed == 0 ? 0 : 1;
}
