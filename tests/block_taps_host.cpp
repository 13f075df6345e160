// block_taps_host.cpp -- block_onepass_taps of the library's srh_block.hpp (the certified one-pass sums with the tap
// products c_t = fma(w_t, l_t, -meanL)*w_t handed in by the row source: the strip kernel's 8-wave form keeps them in LDS per
// tile) compiled for the host and held, bit for bit, to block_onepass: P, Q, U of every candidate and what onepass_finish
// makes of them.  block_onepass is itself held to the select form and the certificate by block_host.cpp.
// A program of its own (tests/test_block_taps_host.py builds it with g++ -O1 -ffp-contract=off, once more with
// -fsanitize=address,undefined, and runs both): usage  block_taps_host <pair file> <radius 2|5>, exit status 0 = every check
// held.  Pair file: int32 w, h; rgba of the left and the right view (w*h*4 bytes each); their masks (w*h bytes each, 1 = in).
//
// Every reference pixel of the left view whose own window is fully usable, against every block of 8 adjacent columns of
// its row in the right view whose 8 windows are fully usable; weights from the oracle, geodesic and adaptive.  The products
// are built once per pixel by the two operations of block_onepass, in its order, as the kernel's per-tile fill does.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "srh_ncc.hpp"
#include "srh_wta.hpp"
#include "srh_block.hpp"

extern "C" {
#include "sr_oracle.h"
void f32r_gray_plane(const sro_image *img, double *out);
}

namespace {

const int PAD = 8;                  // NaN border of the padded planes: radius 5 + slack
const int NCB = 8;

long n_checked = 0, n_failed = 0;

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

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

// The row sources: window row `row` of the other view's segment at r + row*rstride, the weights row-major at w + row*WS;
// the reference view's taps at l + row*lstride (block_onepass) or the products row-major at c + row*WP (block_onepass_taps:
// rows padded to an even count like the kernel's plane, the pad poisoned).  The hook counts what it is given.
template <int WS>
struct ArrayRows {
	static constexpr bool LDS_WAIT = false;
	const double *r; int rstride;
	const double *l; int lstride;
	const double *w;
	long *units, *rows_open;
	struct Row {
		const double *rp, *wp, *lp;
		void r2(int m, double &a, double &b) const { a = rp[2*m]; b = rp[2*m + 1]; }
		void w2(int m, double &a, double &b) const { a = wp[2*m]; b = wp[2*m + 1]; }
		double w(int col) const { return wp[col]; }
		double l(int col) const { return lp[col]; }
	};
	Row row(int row) const { return Row{ r + (size_t)row*rstride, w + row*WS, l + (size_t)row*lstride }; }
	int row_begin(int u) const { *units += u; ++*rows_open; return u; }
	void row_end(int seen) const { if (seen > 0) --*rows_open; }
};

template <int WS>
struct ArrayTapRows {
	static constexpr bool LDS_WAIT = false;
	static constexpr int WP = (WS + 1) & ~1;
	const double *r; int rstride;
	const double *c;
	const double *w;
	long *units, *rows_open;
	struct Row {
		const double *rp, *wp, *cp;
		void r2(int m, double &a, double &b) const { a = rp[2*m]; b = rp[2*m + 1]; }
		void w2(int m, double &a, double &b) const { a = wp[2*m]; b = wp[2*m + 1]; }
		double w(int col) const { return wp[col]; }
		void c2(int m, double &a, double &b) const { a = cp[2*m]; b = cp[2*m + 1]; }
		double c(int col) const { return cp[col]; }
	};
	Row row(int row) const { return Row{ r + (size_t)row*rstride, w + row*WS, c + row*WP }; }
	int row_begin(int u) const { *units += u; ++*rows_open; return u; }
	void row_end(int seen) const { if (seen > 0) --*rows_open; }
};

struct Tally { long pixels = 0, blocks = 0, cert = 0, uncert = 0; };

template <int R>
void run(const sro_image &left, const sro_image &right, const Padded &L, const Padded &Rp, sro_params p, Tally &t)
{
	constexpr int WS = 2*R + 1, T = WS*WS, WP = ArrayTapRows<WS>::WP;
	p.window_radius = R;
	srh_params P;
	std::memset(&P, 0, sizeof P);
	P.window_radius = R;
	P.weight_kind = p.weight_kind == SRO_WEIGHT_GEODESIC ? SRH_WEIGHT_GEODESIC : SRH_WEIGHT_ADAPTIVE;
	P.geodesic_sigma = p.geodesic_sigma; P.adaptive_color_sigma = p.adaptive_color_sigma;
	P.bad_ret = p.bad_ret; P.max_color_diff = p.max_color_diff; P.peak_threshold = p.peak_threshold;
	P.wta_margin = p.wta_margin; P.second_best_factor = p.second_best_factor;
	const srh::CertBound cb = srh::cert_bound(P);
	if (!cb.ok) { std::fprintf(stderr, "cert_bound refuses the parameters\n"); ++n_failed; return; }
	const int W = left.w, H = left.h, SP = L.stride, SPR = Rp.stride;
	std::vector<double> w(T), c((size_t)WS*WP);
	std::vector<char> colok(right.w);
	for (int y = 0; y < H; ++y) {
		// columns of the other view usable on every window row
		for (int cx = 0; cx < right.w; ++cx) {
			bool ok = true;
			for (int row = 0; row < WS; ++row) { const double v = *Rp.at(cx, y - R + row); ok = ok && v == v; }
			colok[cx] = ok;
		}
		for (int x = 0; x < W; ++x) {
			sro_weights(&left, x, y, &p, w.data());
			const double *lp = L.at(x - R, y - R);
			const srh::PixelConstants pc = srh::pixel_constants<WS, true>([&](int row, double *gl, double *wt) {
				for (int col = 0; col < WS; ++col) { gl[col] = lp[(size_t)row*SP + col]; wt[col] = w[row*WS + col]; }
			}, p.weight_cutoff, true);
			if (!pc.all) continue;                             // the fast form's precondition: every tap of the pixel's own window usable
			++t.pixels;
			// the pixel's products, once: a = fma(w, l, -meanL), c = a*w -- block_onepass's two operations
			for (int row = 0; row < WS; ++row) {
				for (int col = 0; col < WS; ++col) {
					const double a = __builtin_fma(w[row*WS + col], lp[(size_t)row*SP + col], -pc.mL);
					c[(size_t)row*WP + col] = a*w[row*WS + col];
				}
				for (int col = WS; col < WP; ++col) c[(size_t)row*WP + col] = NAN;   // never part of a sum
			}
			const double sig3 = cb.sigma3(pc.s2), itw = 1.0/pc.tw;             // (pconst slot 3: pconst_store)
			for (int c0 = R; c0 + NCB - 1 + R < right.w; ++c0) {
				bool usable = true;
				for (int k = c0 - R; k <= c0 + NCB - 1 + R; ++k) usable = usable && colok[k];
				if (!usable) continue;
				++t.blocks;
				long units = 0, rows_open = 0;
				const ArrayRows<WS> src{ Rp.at(c0 - R, y - R), SPR, lp, SP, w.data(), &units, &rows_open };
				double Ps[NCB], Qs[NCB], Us[NCB], Pt[NCB], Qt[NCB], Ut[NCB];
				srh::block_onepass<WS, NCB>(src, pc.mL, Ps, Qs, Us);
				units = 0;
				const ArrayTapRows<WS> taps{ Rp.at(c0 - R, y - R), SPR, c.data(), w.data(), &units, &rows_open };
				srh::block_onepass_taps<WS, NCB>(taps, Pt, Qt, Ut);
				expect(units == 4L*WS && rows_open == 0, "row hook: 4 units per window row", R, x, y, c0, (double)units, 4.0*WS);
				for (int j = 0; j < NCB; ++j) {
					expect(same_bits(Pt[j], Ps[j]), "P", R, x, y, c0 + j, Pt[j], Ps[j]);
					expect(same_bits(Qt[j], Qs[j]), "Q", R, x, y, c0 + j, Qt[j], Qs[j]);
					expect(same_bits(Ut[j], Us[j]), "U", R, x, y, c0 + j, Ut[j], Us[j]);
					bool oks, okt;
					const double vs = srh::onepass_finish(Ps[j], Qs[j], Us[j], pc.sa, itw, pc.s2, (double)T, sig3, cb.zmax2, oks);
					const double vt = srh::onepass_finish(Pt[j], Qt[j], Ut[j], pc.sa, itw, pc.s2, (double)T, sig3, cb.zmax2, okt);
					expect(same_bits(vt, vs) && okt == oks, "finished value and certificate", R, x, y, c0 + j, vt, vs);
					++(oks ? t.cert : t.uncert);
				}
			}
		}
	}
}

}  // namespace

int main(int argc, char **argv)
{
	const int R = argc == 3 ? std::atoi(argv[2]) : 0;
	if (argc != 3 || (R != 2 && R != 5)) { std::fprintf(stderr, "usage: block_taps_host <pair file> <radius 2|5>\n"); return 2; }
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

	Tally t;
	for (int kind = 0; kind < 2; ++kind) {
		sro_params p;
		sro_params_twoview_defaults(&p);
		p.weight_kind = kind == 0 ? SRO_WEIGHT_GEODESIC : SRO_WEIGHT_ADAPTIVE;
		if (R == 2) run<2>(left, right, L, Rp, p, t); else run<5>(left, right, L, Rp, p, t);
	}
	std::printf("%dx%d r=%d: %ld checks, %ld failed; %ld pixels, %ld blocks; one-pass: %ld certified, %ld uncertified\n",
	            wh[0], wh[1], R, n_checked, n_failed, t.pixels, t.blocks, t.cert, t.uncert);
	if (t.blocks == 0) { std::fprintf(stderr, "no block met the fast form's precondition\n"); return 1; }
	// block_onepass certifies every candidate of these pairs: none is left out of the comparison of the finished values
	if (t.uncert != 0) { std::fprintf(stderr, "%ld candidates uncertified: the pair is not the one this test is written for\n", t.uncert); return 1; }
	return n_failed == 0 ? 0 : 1;
}
