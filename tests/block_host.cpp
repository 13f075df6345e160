// block_host.cpp -- the library's srh_block.hpp (stereoreconstruction_amd/csrc: the fast-form block sweeps of the TwoView NCC
// cost, their finishes and the store rule) compiled for the host and held
//   * to ncc_select_cost of srh_ncc.hpp, bit for bit: the exact two sweeps over the whole window and over clipped row
//     ranges (ncc_select_cost is itself held to the oracle by ncc_host.cpp);
//   * to the certificate of srh_wta.hpp: a candidate the fused two sweeps or the one-pass form certify lies within e0 of
//     the exact cost, and block_stored returns NaN, the clamp or the value by its rule.
// A program of its own (tests/test_block_host.py builds it with g++ -O1 -ffp-contract=off, once more with
// -fsanitize=address,undefined, and runs both): usage  block_host <pair file> <radius 2|5>, exit status 0 = every check held.
// Pair file: int32 w, h; rgba of the left and the right view (w*h*4 bytes each); their masks (w*h bytes each, 1 = in).
//
// Every reference pixel of the left view whose own window is fully usable, against every block of 8 adjacent columns of
// its row in the right view whose 8 windows are fully usable; weights from the oracle, geodesic and adaptive.  The row
// source is a plain-array one: pointers and strides into NaN-bordered planes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

// The row source: window row `row` of the other view's segment at r + row*rstride, of the reference view at l + row*lstride,
// the weights row-major at w + row*WS.  The hook counts what it is given: one call pair per window row.
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

struct Tally { long pixels = 0, blocks = 0, cert[2] = {0, 0}, uncert[2] = {0, 0}, clamped[2] = {0, 0}; };   // [0] fused two sweeps, [1] one-pass

// what block_stored must return for a certified form
void expect_store_rule(const char *what, int R, int x, int y, int c, double v, bool certified, const srh::CertBound &cb, double clamp, Tally &t, int form) {
	const double st = srh::block_stored<true>(v, certified, cb.m_hi, clamp);
	if (!certified) { expect(st != st, what, R, x, y, c, st, NAN); ++t.uncert[form]; return; }
	++t.cert[form];
	if (v > cb.m_hi) { expect(same_bits(st, clamp), what, R, x, y, c, st, clamp); ++t.clamped[form]; }
	else expect(same_bits(st, v), what, R, x, y, c, st, v);
}

template <int R>
void run(const sro_image &left, const sro_image &right, const Padded &L, const Padded &Rp, sro_params p, Tally &t)
{
	constexpr int WS = 2*R + 1, T = WS*WS;
	static const int RANGES[3][2] = { { 0, WS }, { 2, WS }, { 0, WS - 3 } };
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
	const double clamp = p.max_color_diff;
	const int W = left.w, H = left.h, SP = L.stride, SPR = Rp.stride;
	std::vector<double> w(T);
	std::vector<double> sel[3];
	std::vector<char> colok(right.w);
	for (int k = 0; k < 3; ++k) sel[k].resize(right.w);
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
			auto rows_l = [&](int row, double *gl, double *wt) {
				for (int col = 0; col < WS; ++col) { gl[col] = lp[(size_t)row*SP + col]; wt[col] = w[row*WS + col]; }
			};
			srh::PixelConstants pc[3];
			for (int k = 0; k < 3; ++k) pc[k] = srh::pixel_constants<WS, true>(rows_l, p.weight_cutoff, true, RANGES[k][0], RANGES[k][1]);
			if (!pc[0].all) continue;                          // the fast form's precondition: every tap of the pixel's own window usable
			++t.pixels;
			// the select form's cost of every column, over the three row ranges (rows left out: taps NaN)
			for (int cx = R; cx + R < right.w; ++cx) {
				const double *rp = Rp.at(cx - R, y - R);
				for (int k = 0; k < 3; ++k) {
					const int ra = RANGES[k][0], rb = RANGES[k][1];
					sel[k][cx] = srh::ncc_select_cost<WS>([&](int row, double *gl, double *gr, double *wt) {
						const bool in = row >= ra && row < rb;
						for (int col = 0; col < WS; ++col) {
							gl[col] = in ? lp[(size_t)row*SP + col] : NAN; gr[col] = in ? rp[(size_t)row*SPR + col] : NAN; wt[col] = w[row*WS + col];
						}
					}, p.weight_cutoff, p.bad_ret, clamp);
				}
			}
			const double sig3 = cb.sigma3(pc[0].s2), itw = 1.0/pc[0].tw;      // (pconst slot 3: pconst_store)
			for (int c0 = R; c0 + NCB - 1 + R < right.w; ++c0) {
				bool usable = true;
				for (int k = c0 - R; k <= c0 + NCB - 1 + R; ++k) usable = usable && colok[k];
				if (!usable) continue;
				++t.blocks;
				long units = 0, rows_open = 0;
				const ArrayRows<WS> src{ Rp.at(c0 - R, y - R), SPR, lp, SP, w.data(), &units, &rows_open };
				// ---- exact two sweeps, whole window and clipped row ranges: the select form's bits
				double vex[NCB];
				for (int k = 0; k < 3; ++k) {
					const int ra = RANGES[k][0], rb = RANGES[k][1];
					double s1[NCB], s3[NCB];
					units = 0;
					srh::block_two_sweeps<WS, NCB, false>(src, ra, rb, pc[k].mL, pc[k].tw, s1, s3);
					expect(units == 4L*(rb - ra) && rows_open == 0, "row hook: 1 + 3 units per window row", R, x, y, c0, (double)units, 4.0*(rb - ra));
					for (int j = 0; j < NCB; ++j) {
						const double v = srh::two_sweep_finish(s1[j], pc[k].s2, s3[j]);
						const double st = srh::block_stored<false>(v, true, cb.m_hi, clamp);
						expect(same_bits(st, sel[k][c0 + j]), k == 0 ? "exact two sweeps" : k == 1 ? "rows [2, WS)" : "rows [0, WS - 3)", R, x, y, c0 + j, st, sel[k][c0 + j]);
						if (k == 0) vex[j] = v;
					}
				}
				// ---- fused two sweeps
				{
					double s1[NCB], s3[NCB];
					srh::block_two_sweeps<WS, NCB, true>(src, 0, WS, pc[0].mL, pc[0].tw, s1, s3);
					for (int j = 0; j < NCB; ++j) {
						const double v = srh::two_sweep_finish(s1[j], pc[0].s2, s3[j]);
						const bool certified = s3[j] >= sig3;
						if (certified) expect(std::fabs(v - vex[j]) <= cb.e0, "fused two sweeps within e0", R, x, y, c0 + j, v, vex[j]);
						expect_store_rule("store rule, fused two sweeps", R, x, y, c0 + j, v, certified, cb, clamp, t, 0);
					}
				}
				// ---- one-pass
				{
					double Ps[NCB], Qs[NCB], Us[NCB];
					units = 0;
					srh::block_onepass<WS, NCB>(src, pc[0].mL, Ps, Qs, Us);
					expect(units == 4L*WS && rows_open == 0, "row hook: 4 units per window row", R, x, y, c0, (double)units, 4.0*WS);
					for (int j = 0; j < NCB; ++j) {
						bool okc;
						const double v = srh::onepass_finish(Ps[j], Qs[j], Us[j], pc[0].sa, itw, pc[0].s2, (double)T, sig3, cb.zmax2, okc);
						if (okc) expect(std::fabs(v - vex[j]) <= cb.e0, "one-pass within e0", R, x, y, c0 + j, v, vex[j]);
						expect_store_rule("store rule, one-pass", R, x, y, c0 + j, v, okc, cb, clamp, t, 1);
					}
				}
			}
		}
	}
}

// one flat window (sum2 ~ 0: sigma3 = +inf) against a textured row segment: neither form certifies a candidate
template <int R>
void flat_window()
{
	constexpr int WS = 2*R + 1, T = WS*WS, NR = NCB + WS - 1;
	srh_params P;
	std::memset(&P, 0, sizeof P);
	P.window_radius = R;
	P.weight_kind = SRH_WEIGHT_GEODESIC; P.geodesic_sigma = 50; P.adaptive_color_sigma = 10;
	P.bad_ret = 1000; P.max_color_diff = 120; P.peak_threshold = 0.95; P.wta_margin = 1e-10; P.second_best_factor = 0.95;
	const srh::CertBound cb = srh::cert_bound(P);
	std::vector<double> l((size_t)WS*WS, 100.0), w((size_t)WS*WS, 1.0), r((size_t)WS*NR);
	for (int row = 0; row < WS; ++row)
		for (int k = 0; k < NR; ++k) r[(size_t)row*NR + k] = (double)((row*37 + k*11) % 251);
	const srh::PixelConstants pc = srh::pixel_constants<WS, true>([&](int row, double *gl, double *wt) {
		for (int col = 0; col < WS; ++col) { gl[col] = l[row*WS + col]; wt[col] = w[row*WS + col]; }
	}, 1e-10, true);
	const double sig3 = cb.sigma3(pc.s2);
	expect(pc.all && cb.ok && sig3 == std::numeric_limits<double>::infinity(), "flat window: sigma3 = +inf", R, -1, -1, -1, sig3, INFINITY);
	long units = 0, rows_open = 0;
	const ArrayRows<WS> src{ r.data(), NR, l.data(), WS, w.data(), &units, &rows_open };
	double s1[NCB], s3[NCB], Ps[NCB], Qs[NCB], Us[NCB];
	srh::block_two_sweeps<WS, NCB, true>(src, 0, WS, pc.mL, pc.tw, s1, s3);
	srh::block_onepass<WS, NCB>(src, pc.mL, Ps, Qs, Us);
	for (int j = 0; j < NCB; ++j) {
		bool okc;
		const double v = srh::onepass_finish(Ps[j], Qs[j], Us[j], pc.sa, 1.0/pc.tw, pc.s2, (double)T, sig3, cb.zmax2, okc);
		expect(!(s3[j] >= sig3), "flat window: fused two sweeps certify nothing", R, -1, -1, j, s3[j], sig3);
		expect(!okc, "flat window: one-pass certifies nothing", R, -1, -1, j, v, NAN);
		const double st = srh::block_stored<true>(v, okc, cb.m_hi, P.max_color_diff);
		expect(st != st, "flat window: NaN stored", R, -1, -1, j, st, NAN);
	}
}

// the store rule on values the pairs need not produce: the clamp's neighbourhood, NaN
void store_rule_cases()
{
	const double clamp = 120.0, e0 = 0x1p-26, m_hi = clamp + e0, nan = NAN;
	const double below = std::nextafter(clamp, 0.0), in_gap = clamp + e0/2, above = std::nextafter(m_hi, 1e9);
	// exact forms: twoviewstereo.cpp:976, `v < clamp ? v : clamp` (a NaN value becomes the clamp)
	expect(same_bits(srh::block_stored<false>(below, true, m_hi, clamp), below), "exact store: below the clamp", 0, -1, -1, 0, 0, 0);
	expect(same_bits(srh::block_stored<false>(clamp, true, m_hi, clamp), clamp), "exact store: the clamp", 0, -1, -1, 1, 0, 0);
	expect(same_bits(srh::block_stored<false>(in_gap, false, m_hi, clamp), clamp), "exact store: above the clamp", 0, -1, -1, 2, 0, 0);
	expect(same_bits(srh::block_stored<false>(nan, true, m_hi, clamp), clamp), "exact store: NaN", 0, -1, -1, 3, 0, 0);
	// certified forms: NaN when uncertified whatever the value; the clamp above clamp + e0; else the value as it is
	for (double v : { below, clamp, in_gap, m_hi, above, 254.0 }) {
		const double un = srh::block_stored<true>(v, false, m_hi, clamp), ce = srh::block_stored<true>(v, true, m_hi, clamp);
		expect(un != un, "certified store: uncertified is NaN", 0, -1, -1, 4, un, nan);
		expect(same_bits(ce, v > m_hi ? clamp : v), "certified store: clamp above m_hi, else the value", 0, -1, -1, 5, ce, v);
	}
	expect(same_bits(srh::block_stored<true>(m_hi, true, m_hi, clamp), m_hi) && same_bits(srh::block_stored<true>(above, true, m_hi, clamp), clamp),
	       "certified store: m_hi itself is kept, the next value is the clamp", 0, -1, -1, 6, 0, 0);
}

}  // namespace

int main(int argc, char **argv)
{
	const int R = argc == 3 ? std::atoi(argv[2]) : 0;
	if (argc != 3 || (R != 2 && R != 5)) { std::fprintf(stderr, "usage: block_host <pair file> <radius 2|5>\n"); return 2; }
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
	if (R == 2) flat_window<2>(); else flat_window<5>();
	store_rule_cases();
	std::printf("%dx%d r=%d: %ld checks, %ld failed; %ld pixels, %ld blocks; fused two sweeps: %ld certified (%ld stored as the clamp), %ld uncertified; "
	            "one-pass: %ld certified (%ld stored as the clamp), %ld uncertified\n", wh[0], wh[1], R, n_checked, n_failed, t.pixels, t.blocks,
	            t.cert[0], t.clamped[0], t.uncert[0], t.cert[1], t.clamped[1], t.uncert[1]);
	if (t.blocks == 0) { std::fprintf(stderr, "no block met the fast form's precondition\n"); return 1; }
	// a form that certifies fewer candidates than it leaves uncertified on a textured pair is not the kernels' form
	for (int form = 0; form < 2; ++form)
		if (t.cert[form] < t.uncert[form]) { std::fprintf(stderr, "%s certifies fewer candidates than it leaves uncertified\n", form == 0 ? "fused two sweeps" : "one-pass"); return 1; }
	return n_failed == 0 ? 0 : 1;
}
