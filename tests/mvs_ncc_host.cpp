// mvs_ncc_host.cpp -- the library's srh_mvs_ncc.hpp (stereoreconstruction_amd/csrc) compiled for the host and held to the
// oracle, bit for bit.  A program of its own (tests/test_mvs_ncc_host.py builds it with g++ -O1 -ffp-contract=off, once
// more with -fsanitize=address,undefined, and runs both): usage  mvs_ncc_host <pair file>..., exit status 0 = every check
// held and every case met what it is there for (counted over all the files).
// Pair file: int32 w, h; rgba of the two views (w*h*4 bytes each); their masks (w*h bytes each, 1 = in).
//
//   mvs_select_cost / mvs_select_cost_n against sro_mvs_cost_ncc: every reference pixel against every candidate (cx, cy)
//       in [-3, w + 3) x [-3, h + 3), radius 2 and 3, geodesic and adaptive weights, once with a cut-off that removes
//       taps; the taps fed the three ways the kernels know: NaN-bordered planes (mvs_tap), unconditional loads from
//       clamped addresses plus a mask (mvs_cost_select), and a reference side whose usability was settled beforehand
//       (an okl array).
//   mvs_select_cost_masked (mvs_unit_general's own statement: raw clamped loads and a mask) against the same.
//   mvs_unit_constants + mvs_fast_cost (whole, and row by row) against mvs_select_cost wherever the unit is `all` and the
//       candidate's window lies inside the image.
//   mvs_peaks_insert against "sort the pairs, keep the last K"; mvs_peak_better against the same with K = 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "srh_mvs_ncc.hpp"

extern "C" {
#include "sr_oracle.h"
}

namespace {

const int PAD = 8;                  // NaN border of the padded planes: radius 3 + three pixels outside + slack
const int OUTSIDE = 3;

long n_checked = 0, n_failed = 0;
// what the cases are there for
long n_tw_return = 0, n_den_return = 0, n_cut_taps = 0, n_all_units = 0, n_other_units = 0, n_cost_ties = 0;

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

void expect(bool ok, const char *what, int R, int x, int y, int cx, int cy, double got, double want) {
	++n_checked;
	if (ok) return;
	if (++n_failed <= 20) std::fprintf(stderr, "FAIL %s: r=%d pixel (%d, %d) candidate (%d, %d): got %.17g want %.17g\n", what, R, x, y, cx, cy, got, want);
}

struct Plane {                       // gray values (RGBA::toGray of every pixel, masked or not: the free cost_ncc reads pixel())
	int w, h, stride;
	std::vector<double> v, padded;
	Plane(const sro_image &img) : w(img.w), h(img.h), stride(img.w + 2*PAD), v((size_t)img.w*img.h), padded((size_t)(img.w + 2*PAD)*(img.h + 2*PAD), NAN) {
		for (int y = 0; y < h; ++y)
			for (int x = 0; x < w; ++x) {
				const uint8_t *p = img.rgba + ((size_t)y*w + x)*4;
				v[(size_t)y*w + x] = padded[(size_t)(y + PAD)*stride + (x + PAD)] = sro_to_gray(p[0], p[1], p[2]);
			}
	}
	double nan_outside(int x, int y) const { return padded[(size_t)(y + PAD)*stride + (x + PAD)]; }
	// an unconditional load from the clamped address; ok = the address was not clamped
	double clamped(int x, int y, bool &ok) const {
		const int xc = x < 0 ? 0 : (x >= w ? w - 1 : x), yc = y < 0 ? 0 : (y >= h ? h - 1 : y);
		ok = xc == x && yc == y;
		return v[(size_t)yc*w + xc];
	}
};

// which return the reference takes for this pair of windows (the guarded sums of multiviewstereo.cpp:113-189 once more,
// for the tallies only)
void classify(const Plane &L, const Plane &Rp, const double *w, int R, double cutoff, int x, int y, int cx, int cy) {
	const int WS = 2*R + 1;
	double mL = 0, mR = 0, tw = 0;
	for (int row = 0; row < WS; ++row)
		for (int col = 0; col < WS; ++col) {
			const double gl = L.nan_outside(x - R + col, y - R + row), gr = Rp.nan_outside(cx - R + col, cy - R + row), wt = w[row*WS + col];
			if (gl == gl && gr == gr && wt > cutoff) { mL += wt*gl; mR += wt*gr; tw += wt; }
		}
	if (tw < 1e-10) { ++n_tw_return; return; }
	mL /= tw; mR /= tw;
	double s2 = 0, s3 = 0;
	for (int row = 0; row < WS; ++row)
		for (int col = 0; col < WS; ++col) {
			const double gl = L.nan_outside(x - R + col, y - R + row), gr = Rp.nan_outside(cx - R + col, cy - R + row), wt = w[row*WS + col];
			if (gl == gl && gr == gr && wt > cutoff) { s2 += (wt*gl - mL)*(wt*gl - mL); s3 += (wt*gr - mR)*(wt*gr - mR); }
		}
	if (s2 * s3 < 1e-10) ++n_den_return;
}

template <int R>
void run(const sro_image &ref, const sro_image &oth, const Plane &L, const Plane &Rp, sro_params p)
{
	constexpr int WS = 2*R + 1, T = WS*WS;
	p.window_radius = R;
	const double cutoff = p.weight_cutoff;
	const int W = ref.w, H = ref.h;
	std::vector<double> w(T);
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) {
			sro_weights(&ref, x, y, &p, w.data());
			// the reference side, as mvs_unit_general holds it (clamped loads) and with its usability settled beforehand
			double gl_n[T], gl_c[T], gl_ok[T];
			bool okl_a[T];
			bool usable = true;
			double sum_w = 0, w_arr[T];
			for (int t = 0; t < T; ++t) w_arr[t] = w[t];
			for (int t = 0; t < T; ++t) {
				bool in;
				const double v = L.clamped(x - R + t % WS, y - R + t / WS, in);
				gl_c[t] = in ? v : NAN;
				gl_n[t] = L.nan_outside(x - R + t % WS, y - R + t / WS);
				const bool okl = in && w[t] > cutoff;
				gl_ok[t] = okl ? v : NAN;
				okl_a[t] = okl;
				usable = usable && okl;
				sum_w += w[t];
				if (!(w[t] > cutoff)) ++n_cut_taps;
			}

			// ---- the unit's constants: weights in a plain array (registers) and in a strided column (the list kernel's LDS)
			double wreg[T], a[T], wcol[T*3], a2[T], az[T];
			const auto tap = [&](int t, double &wt, double &gl) { wt = w[t]; gl = L.nan_outside(x - R + t % WS, y - R + t / WS); };
			const srh::MvsUnit u = srh::mvs_unit_constants<T, false>(tap, [&](int t) -> double & { return wreg[t]; }, a, cutoff, true);
			const srh::MvsUnit u2 = srh::mvs_unit_constants<T, false>(tap, [&](int t) -> double & { return wcol[3*t + 1]; }, a2, cutoff, true);
			const srh::MvsUnit uz = srh::mvs_unit_constants<T, true>(tap, [&](int t) -> double & { return wreg[t]; }, az, cutoff, true);
			double wf[T], af[T];
			const srh::MvsUnit uf = srh::mvs_unit_constants<T, true>(tap, [&](int t) -> double & { return wf[t]; }, af, cutoff, false);
			expect(u.all == (usable && !(sum_w < 1e-10)), "all = every tap usable", R, x, y, 0, 0, u.all, usable);
			expect(same_bits(u.tw, sum_w), "unit tw", R, x, y, 0, 0, u.tw, sum_w);
			expect(u2.all == u.all && same_bits(u2.tw, u.tw) && same_bits(u2.s2, u.s2) && uz.all == u.all && same_bits(uz.s2, u.s2), "unit constants, other storage", R, x, y, 0, 0, u2.s2, u.s2);
			expect(!uf.all && same_bits(uf.s2, 0.0), "a false seed", R, x, y, 0, 0, uf.s2, 0.0);
			for (int t = 0; t < T; ++t) {
				expect(same_bits(wreg[t], w[t]) && same_bits(wcol[3*t + 1], w[t]), "weights through the caller's storage", R, x, y, t, 0, wreg[t], w[t]);
				expect(same_bits(a2[t], a[t]), "a_t, other storage", R, x, y, t, 0, a2[t], a[t]);
				expect(same_bits(az[t], u.all ? a[t] : 0.0), "a_t with ZERO_A (0 when not all)", R, x, y, t, 0, az[t], a[t]);
				expect(same_bits(af[t], 0.0), "a_t = 0 (ZERO_A, false seed)", R, x, y, t, 0, af[t], 0.0);
				if (!u.all) expect(same_bits(a[t], L.nan_outside(x - R + t % WS, y - R + t / WS)), "a_t left as gray", R, x, y, t, 0, a[t], 0.0);
			}
			if (u.all) ++n_all_units; else ++n_other_units;

			for (int cy = -OUTSIDE; cy < oth.h + OUTSIDE; ++cy)
				for (int cx = -OUTSIDE; cx < oth.w + OUTSIDE; ++cx) {
					const double want = sro_mvs_cost_ncc(&ref, &oth, w.data(), &p, x, y, cx, cy);
					if (want == 0) classify(L, Rp, w.data(), R, cutoff, x, y, cx, cy);   // (either early return gives 0)
					// the candidate's window fetched the two ways the kernels fetch it
					double gr_n[T], gr_c[T], gr_raw[T];
					bool ok_m[T];
					for (int t = 0; t < T; ++t) {
						bool in;
						const double v = Rp.clamped(cx - R + t % WS, cy - R + t / WS, in);
						gr_c[t] = in ? v : NAN;
						gr_raw[t] = v;
						ok_m[t] = okl_a[t] && in;
						gr_n[t] = Rp.nan_outside(cx - R + t % WS, cy - R + t / WS);
					}
					// 1. NaN for outside on both sides (mvs_tap)
					const double nan_t = srh::mvs_select_cost<WS>([&](int row, double *gl, double *gr, double *wt) {
						for (int col = 0; col < WS; ++col) { gl[col] = gl_n[row*WS + col]; gr[col] = gr_n[row*WS + col]; wt[col] = w[row*WS + col]; }
					}, cutoff);
					const double nan_n = srh::mvs_select_cost_n(WS, [&](int row, int col, double &gl, double &gr, double &wt) {
						gl = gl_n[row*WS + col]; gr = gr_n[row*WS + col]; wt = w[row*WS + col];
					}, cutoff);
					// 2. clamped address plus mask on both sides (mvs_unit_general, mvs_cost_select)
					const double cl_t = srh::mvs_select_cost<WS>([&](int row, double *gl, double *gr, double *wt) {
						for (int col = 0; col < WS; ++col) { gl[col] = gl_c[row*WS + col]; gr[col] = gr_c[row*WS + col]; wt[col] = w[row*WS + col]; }
					}, cutoff);
					const double cl_n = srh::mvs_select_cost_n(WS, [&](int row, int col, double &gl, double &gr, double &wt) {
						gl = gl_c[row*WS + col]; gr = gr_c[row*WS + col]; wt = w[row*WS + col];
					}, cutoff);
					// 3. the reference side's usability as an array made once per unit
					const double ok_t = srh::mvs_select_cost<WS>([&](int row, double *gl, double *gr, double *wt) {
						for (int col = 0; col < WS; ++col) { gl[col] = gl_ok[row*WS + col]; gr[col] = gr_n[row*WS + col]; wt[col] = w[row*WS + col]; }
					}, cutoff);
					const double ok_n = srh::mvs_select_cost_n(WS, [&](int row, int col, double &gl, double &gr, double &wt) {
						gl = gl_ok[row*WS + col]; gr = gr_c[row*WS + col]; wt = w[row*WS + col];
					}, cutoff);
					// mvs_unit_general's statement: the raw clamped loads and a mask
					const double masked = srh::mvs_select_cost_masked<T>(w_arr, gl_c, gr_raw, ok_m);
					expect(same_bits(masked, want), "mvs_select_cost_masked", R, x, y, cx, cy, masked, want);
					const double got[6] = { nan_t, nan_n, cl_t, cl_n, ok_t, ok_n };
					static const char *const feed[6] = { "mvs_select_cost, NaN outside", "mvs_select_cost_n, NaN outside", "mvs_select_cost, clamped + mask",
					                                     "mvs_select_cost_n, clamped + mask", "mvs_select_cost, okl array", "mvs_select_cost_n, okl array" };
					for (int i = 0; i < 6; ++i) expect(same_bits(got[i], want), feed[i], R, x, y, cx, cy, got[i], want);

					// ---- the fast form
					if (!(u.all && cx - R >= 0 && cy - R >= 0 && cx + R < oth.w && cy + R < oth.h)) continue;
					double g[T], g2[T];
					for (int t = 0; t < T; ++t) g[t] = g2[t] = gr_n[t];
					const double fast = srh::mvs_fast_cost<T>([&](int t) { return wreg[t]; }, a, g, u.tw, u.s2);
					// row by row, the weights from the strided column
					double mR = 0, s1 = 0, s3 = 0;
					for (int row = 0; row < WS; ++row) srh::mvs_fast_products<WS>([&](int t) { return wcol[3*t + 1]; }, g2, row*WS, mR);
					mR /= u2.tw;
					for (int row = 0; row < WS; ++row) srh::mvs_fast_sums<WS>(a2, g2, row*WS, mR, s1, s3);
					const double by_rows = srh::mvs_fast_finish(s1, u2.s2 * s3);
					expect(same_bits(fast, nan_t), "mvs_fast_cost against mvs_select_cost", R, x, y, cx, cy, fast, nan_t);
					expect(same_bits(by_rows, nan_t), "fast form row by row", R, x, y, cx, cy, by_rows, nan_t);
				}
		}
}

// ---- peaks
typedef std::pair<double, double> Pair;

void check_peaks(const std::vector<Pair> &pairs, int K, const char *order)
{
	std::vector<double> pk(2*K);
	srh::mvs_peaks_init(pk.data(), K);
	std::vector<Pair> seen(K, Pair(0.0, -1.0));                  // K x (0, -1), multiviewstereo.cpp:553
	for (int k = 0; k < K; ++k) expect(pk[2*k] == 0.0 && pk[2*k + 1] == -1.0, "mvs_peaks_init", K, k, 0, 0, 0, pk[2*k], 0.0);
	Pair best(0.0, -1.0);
	for (size_t i = 0; i < pairs.size(); ++i) {
		const double c = pairs[i].first, z = pairs[i].second;
		srh::mvs_peaks_insert(pk.data(), K, c, z);
		if (c == best.first && z != best.second) ++n_cost_ties;
		if (srh::mvs_peak_better(c, z, best.first, best.second)) best = pairs[i];
		seen.push_back(pairs[i]);
		if (i < 40 || i % 97 == 0 || i + 1 == pairs.size()) {
			std::vector<Pair> s(seen);
			std::sort(s.begin(), s.end());
			for (int k = 0; k < K; ++k) {
				const Pair &want = s[s.size() - K + k];
				expect(same_bits(pk[2*k], want.first) && same_bits(pk[2*k + 1], want.second), order, K, (int)i, k, 0, 0, pk[2*k], want.first);
			}
			expect(same_bits(best.first, s.back().first) && same_bits(best.second, s.back().second), "mvs_peak_better against the sort's back()", K, (int)i, 0, 0, 0, best.first, s.back().first);
		}
	}
}

void run_peaks()
{
	// a few thousand pairs from a small set of values: cost ties and full ties
	const double costs[] = { 0.951, 0.96, 0.97, 0.975, 0.99, 1.0 }, depths[] = { 0.5, 1.0, 1.25, 2.0, 3.5 };
	std::vector<Pair> pairs;
	uint32_t s = 12345u;
	for (int i = 0; i < 3000; ++i) {
		s = s*1664525u + 1013904223u;
		const double c = costs[(s >> 8) % 6];
		s = s*1664525u + 1013904223u;
		pairs.push_back(Pair(c, depths[(s >> 8) % 5]));
	}
	std::vector<Pair> rev(pairs.rbegin(), pairs.rend());
	for (int K : { 1, 3, 9 }) {
		check_peaks(pairs, K, "mvs_peaks_insert, first order");
		check_peaks(rev, K, "mvs_peaks_insert, reversed order");
	}
}

bool run_file(const char *path)
{
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::perror(path); return false; }
	int32_t wh[2];
	if (std::fread(wh, sizeof wh, 1, f) != 1 || wh[0] <= 0 || wh[1] <= 0 || wh[0] > 4096 || wh[1] > 4096) { std::fclose(f); return false; }
	const size_t n = (size_t)wh[0]*wh[1];
	std::vector<uint8_t> rgba[2] = { std::vector<uint8_t>(4*n), std::vector<uint8_t>(4*n) }, mask[2] = { std::vector<uint8_t>(n), std::vector<uint8_t>(n) };
	const bool ok = std::fread(rgba[0].data(), 1, 4*n, f) == 4*n && std::fread(rgba[1].data(), 1, 4*n, f) == 4*n
	             && std::fread(mask[0].data(), 1, n, f) == n && std::fread(mask[1].data(), 1, n, f) == n;
	std::fclose(f);
	if (!ok) { std::fprintf(stderr, "%s: short file\n", path); return false; }
	const sro_image ref = { wh[0], wh[1], rgba[0].data(), mask[0].data() }, oth = { wh[0], wh[1], rgba[1].data(), mask[1].data() };
	const Plane L(ref), Rp(oth);
	for (int kind = 0; kind < 2; ++kind) {
		sro_params p;
		sro_params_mvs_defaults(&p);
		p.weight_kind = kind == 0 ? SRO_WEIGHT_GEODESIC : SRO_WEIGHT_ADAPTIVE;
		run<2>(ref, oth, L, Rp, p);
		run<3>(ref, oth, L, Rp, p);
	}
	{
		// a cut-off that removes taps: geodesic weights are exp(-distance/sigma), 1 at the centre
		sro_params p;
		sro_params_mvs_defaults(&p);
		p.weight_kind = SRO_WEIGHT_GEODESIC;
		p.weight_cutoff = 0.5;
		run<2>(ref, oth, L, Rp, p);
	}
	return true;
}

}  // namespace

int main(int argc, char **argv)
{
	if (argc < 2) { std::fprintf(stderr, "usage: mvs_ncc_host <pair file>...\n"); return 2; }
	for (int i = 1; i < argc; ++i)
		if (!run_file(argv[i])) return 2;
	run_peaks();
	std::printf("%ld checks, %ld failed; returns through totalWeight %ld, through sum2*sum3 %ld; %ld cut taps; %ld units with every tap usable, "
	            "%ld others; %ld cost ties with different depths\n", n_checked, n_failed, n_tw_return, n_den_return, n_cut_taps,
	            n_all_units, n_other_units, n_cost_ties);
	// the cases must have met what they are there for
	if (n_tw_return == 0 || n_den_return == 0 || n_cut_taps == 0 || n_all_units == 0 || n_other_units == 0 || n_cost_ties == 0) {
		std::fprintf(stderr, "a case met none of what it is there for\n");
		return 1;
	}
	return n_failed == 0 ? 0 : 1;
}
