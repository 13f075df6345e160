// stripframe_host.cpp -- the host-clean part of the library's srh_stripframe.hpp (stereoreconstruction_amd/csrc: the frame of
// the persistent strip kernels) compiled for the host and held to what it stands for:
//   * StripItems::cut / segment: the items of a band cover every (row, tile column) exactly once, none taller than 16 rows
//     or empty, heights non-increasing in item order, nitems = their count;
//   * StripItems::border_rows / cut_border / segment_border: rows [0, t) and [b, nrows) each once, tile columns in the
//     order 0, last, 1, 2, ...;
//   * padded_raster_xy: every raster index maps to one (x, y); "inside" exactly on the W*H image positions, at
//     (y + SRH_PADY)*padded_stride + x + SRH_PADL;
//   * ring_slot: (s0 + row) mod NS;
//   * strip_lane_blocks: the expressions of the kernels it replaced.
// A program of its own (tests/test_stripframe_host.py builds it with g++, once more with -fsanitize=address,undefined, and
// runs both): no arguments, exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "srh_stripframe.hpp"

namespace {

long n_checked = 0, n_failed = 0;

void expect(bool ok, const char *what, int a, int b, int c, int d) {
	++n_checked;
	if (ok) return;
	if (++n_failed <= 20) std::fprintf(stderr, "FAIL %s: %d %d %d %d\n", what, a, b, c, d);
}

void items_cases()
{
	static const int WIDTHS[] = { 1, 31, 32, 33, 65, 320 };
	for (int nrows = 0; nrows <= 70; ++nrows)
		for (int W : WIDTHS) {
			const int tpr = (W + srh::STRIP_TP - 1)/srh::STRIP_TP;
			const srh::StripItems it = srh::StripItems::cut(nrows, W);
			std::vector<int> seen((size_t)nrows*tpr, 0);
			int prev = 16;
			for (int item = 0; item < it.nitems; ++item) {
				int tx = -1, ya = -1, nh = -1;
				it.segment(item, tpr, nrows, tx, ya, nh);
				const bool in = tx >= 0 && tx < tpr && ya >= 0 && nh >= 1 && nh <= 16 && ya + nh <= nrows;
				expect(in, "item inside the band, 1 .. 16 rows", nrows, W, item, nh);
				if (!in) continue;
				expect(nh <= prev, "heights non-increasing in item order", nrows, W, item, nh);
				prev = nh;
				for (int r = ya; r < ya + nh; ++r) ++seen[(size_t)r*tpr + tx];
			}
			long once = 0;
			for (int v : seen) once += v == 1;
			expect(once == (long)nrows*tpr, "every (row, tile column) exactly once", nrows, W, (int)once, nrows*tpr);
			// one item beyond the count would be an empty one or leave the band: nitems is the count
			if (nrows == 0) expect(it.nitems == 0, "no rows: no item", nrows, W, it.nitems, 0);
		}
}

void border_cases()
{
	struct Case { int y0, nrows, H, R; };
	static const Case CASES[] = {
		{ 0, 9, 9, 2 }, { 0, 12, 12, 5 },       // the whole image: top and bottom
		{ 0, 6, 40, 5 }, { 0, 3, 40, 5 },       // top only (the second: nothing but border rows)
		{ 30, 10, 40, 5 }, { 37, 3, 40, 2 },    // bottom only
		{ 10, 12, 40, 5 },                      // neither
		{ 0, 7, 7, 5 }, { 0, 4, 4, 2 },         // an image lower than a window: every row is a border row
	};
	static const int WIDTHS[] = { 1, 33, 65, 320 };
	for (const Case &c : CASES)
		for (int W : WIDTHS) {
			const int tpr = (W + srh::STRIP_TP - 1)/srh::STRIP_TP;
			int t = -1, b = -1;
			srh::StripItems::border_rows(c.y0, c.nrows, c.H, c.R, t, b);
			expect(0 <= t && t <= b && b <= c.nrows, "0 <= t <= b <= nrows", c.y0, c.nrows, t, b);
			// a band row is a border row exactly when the image's top or bottom edge cuts its window
			for (int r = 0; r < c.nrows; ++r) {
				const int y = c.y0 + r;
				expect((r < t || r >= b) == (y < c.R || y > c.H - 2 - c.R), "border rows: y < R or y > H - 2 - R", c.y0, c.H, c.R, r);
			}
			const srh::StripItems it = srh::StripItems::cut_border(t, b, c.nrows, W);
			std::vector<int> seen((size_t)c.nrows*tpr, 0);
			std::vector<int> order;                       // tile columns in the order their first item comes
			for (int item = 0; item < it.nitems; ++item) {
				int tx = -1, ya = -1, nh = -1;
				it.segment_border(item, tpr, c.nrows, tx, ya, nh);
				const bool in = tx >= 0 && tx < tpr && ya >= 0 && nh >= 1 && nh <= srh::STRIP_BROWS && ya + nh <= c.nrows;
				// (one tile column: the "last column" slot of the order names column 0 again -- tpr == 1 has nitems of one column only)
				expect(in, "border item inside the band", c.y0, W, item, nh);
				if (!in) continue;
				if (order.empty() || order.back() != tx) order.push_back(tx);
				for (int r = ya; r < ya + nh; ++r) ++seen[(size_t)r*tpr + tx];
			}
			for (int r = 0; r < c.nrows; ++r)
				for (int tx = 0; tx < tpr; ++tx)
					expect(seen[(size_t)r*tpr + tx] == ((r < t || r >= b) ? 1 : 0), "border rows once, the others never", c.y0, W, r, tx);
			if (it.nitems > 0) {
				expect((int)order.size() == tpr, "every tile column, in one run each", c.y0, W, (int)order.size(), tpr);
				for (int k = 0; k < (int)order.size(); ++k)
					expect(order[k] == (k == 0 ? 0 : k == 1 ? tpr - 1 : k - 1), "tile columns 0, last, 1, 2, ...", c.y0, W, k, order[k]);
			}
		}
}

void raster_cases()
{
	static const int SIZES[][2] = { { 1, 1 }, { 33, 9 }, { 65, 12 } };
	for (const auto &s : SIZES) {
		const int W = s[0], H = s[1], SP = srh::padded_stride(W);
		const size_t n = srh::padded_size(W, H);
		expect(n == (size_t)(W + SRH_PADL + SRH_PADR)*(size_t)(H + 2*SRH_PADY), "padded_size", W, H, (int)n, 0);
		std::vector<int> hit((size_t)W*H, 0);
		long inside = 0;
		for (size_t k = 0; k < n; ++k) {
			int x = 0, y = 0;
			const bool in = srh::padded_raster_xy(k, W, H, x, y);
			// one (x, y) per index: the map inverts
			expect((size_t)(y + SRH_PADY)*SP + (size_t)(x + SRH_PADL) == k && x >= -SRH_PADL && x < W + SRH_PADR, "index <-> (x, y)", W, H, x, y);
			expect(in == (x >= 0 && y >= 0 && x < W && y < H), "inside = an image position", W, H, x, y);
			if (in) { ++inside; ++hit[(size_t)y*W + x]; }
		}
		long once = 0;
		for (int v : hit) once += v == 1;
		expect(inside == (long)W*H && once == (long)W*H, "inside exactly on the W*H image positions", W, H, (int)inside, (int)once);
	}
}

template <int R>
void ring_cases()
{
	constexpr int WS = srh::StripGeom<R>::WS, NS = srh::StripGeom<R>::NS;
	for (int s0 = 0; s0 < NS; ++s0)
		for (int row = 0; row < WS; ++row) expect(srh::ring_slot(s0, row, NS) == (s0 + row) % NS, "ring_slot", R, s0, row, NS);
}

template <bool PAD>
void block_cases()
{
	const int CHUNK = srh::STRIP_CHUNK, NCB = srh::STRIP_NCB;
	for (int cs = 0; cs <= 6; cs += 2)                                      // (the staging origin is even)
		for (int e_min = cs - 3; e_min <= cs + 12; ++e_min)                  // lo of both parities, in front of and behind cs
			for (int e_max = e_min - 2; e_max <= cs + CHUNK + 3; e_max += (e_max > e_min + 20 && e_max < cs + CHUNK - 12) ? 7 : 1) {
				int lo, hi, lo_e, nblocks;
				srh::strip_lane_blocks<PAD>(e_min, e_max, cs, lo, hi, lo_e, nblocks);
				// the kernels' expressions
				const int xlo = e_min > cs ? e_min : cs;
				const int xhi = e_max < cs + CHUNK - 1 ? e_max : cs + CHUNK - 1;
				const int xlo_e = PAD ? (xlo & ~1) : xlo;
				const int xnb = xhi >= xlo ? (xhi - xlo_e + NCB)/NCB : 0;
				expect(lo == xlo && hi == xhi && lo_e == xlo_e && nblocks == xnb, "strip_lane_blocks", cs, e_min, e_max, PAD);
				// and what they are for: the blocks cover [lo, hi], start inside the staged columns, on an even column when PAD
				if (nblocks > 0) {
					expect(lo_e >= cs && lo_e <= lo && lo - lo_e <= (PAD ? 1 : 0) && (!PAD || lo_e % 2 == 0), "first block", cs, e_min, e_max, lo_e);
					expect(lo_e + nblocks*NCB > hi && lo_e + (nblocks - 1)*NCB <= hi && hi < cs + CHUNK, "last block", cs, e_min, e_max, nblocks);
					expect(nblocks <= srh::StripGeom<5>::NBMAX, "nblocks <= NBMAX", cs, e_min, e_max, nblocks);
				}
			}
}

}  // namespace

int main()
{
	items_cases();
	border_cases();
	raster_cases();
	ring_cases<2>();
	ring_cases<5>();
	block_cases<true>();
	block_cases<false>();
	std::printf("stripframe: %ld checks, %ld failed\n", n_checked, n_failed);
	return n_failed == 0 ? 0 : 1;
}
