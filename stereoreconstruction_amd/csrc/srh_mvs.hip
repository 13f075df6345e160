// srh_mvs.hip -- gfx950 kernels of MultiViewStereo's initial estimate.  IEEE double in the reference's operation
// order; built with -ffp-contract=off.  The cost arithmetic and the peak rule are srh_mvs_ncc.hpp's.
//
//   mvs_generic_kernel, mvs_reg_kernel   epipolarCurve + cost_ncc + top-K / best, one thread per pixel
//   mvs_walk_kernel -> mvs_list_cost_kernel / mvs_staged_cost_kernel -> mvs_combine_kernel   the default path, in stages
//   mvs_cross_check_kernel               (#17)
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_mvs_ncc.hpp"

namespace srh {

// ------------------------------------------------------------------ MVS, general geometry
struct MvsVisitor {
	const ViewDev &A, &B;
	const double *wq;
	size_t wstride;
	const srh_params &P;
	const Ray &ray;
	int x, y;
	double bestCost, bestDepth;
	double *peaks;          // top_k (cost, depth) pairs, ascending; may be null
	unsigned n;
	__device__ __forceinline__ void operator()(int cx, int cy) {
		const double cost = mvs_cost(A, B, wq, wstride, P, x, y, cx, cy);
		++n;
		if (cost > P.peak_threshold) {                          // multiviewstereo.cpp:589-594
			const double z = candidate_depth(A.cam, B.cam, P, ray, cx, cy);
			// std::sort of (cost, depth) pairs, keep the last K, result = back()
			if (mvs_peak_better(cost, z, bestCost, bestDepth)) { bestCost = cost; bestDepth = z; }
			if (peaks) mvs_peaks_insert(peaks, P.top_k, cost, z);
		}
	}
};

__global__ void mvs_generic_kernel(const ViewDev *__restrict__ views, int ref,
                                   NeighList nl, int nneigh, srh_params P,
                                   int y0, int nrows, const double *__restrict__ wbuf, size_t wstride,
                                   double *__restrict__ peaks, Counters *__restrict__ cnt)
{
	const ViewDev &A = views[ref];
	const int W = A.w;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	unsigned n_eval = 0, n_pix = 0;
	if (q < (size_t)nrows*W) {
		const int x = (int)(q % W), y = y0 + (int)(q / W);
		const size_t pv = (size_t)y*W + x;
		double depth = __builtin_inf();                         // multiviewstereo.cpp:559
		double *pk = peaks ? peaks + pv*(size_t)P.top_k*2 : nullptr;
		if (pk) mvs_peaks_init(pk, P.top_k);
		if (A.mask[pv] == 1) {
			n_pix = 1;
			const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
			const int T = (2*P.window_radius + 1)*(2*P.window_radius + 1);
			MvsVisitor vis = { A, A, wbuf + wbuf_offset(W, T, (int)(q / W), x), wstride, P, ray, x, y, 0.0, -1.0, pk, 0 };
			for (int ni = 0; ni < nneigh; ++ni) {
				const int v2 = nl.n[ni];
				const ViewDev &B = views[v2];
				MvsVisitor vb = { A, B, vis.wq, wstride, P, ray, x, y, vis.bestCost, vis.bestDepth, pk, vis.n };
				walk_curve<true>(ray, A.cam, B, P, vb);
				vis.bestCost = vb.bestCost; vis.bestDepth = vb.bestDepth; vis.n = vb.n;
			}
			n_eval = vis.n;
			depth = vis.bestDepth;                              // peakPairs[y][x].back().second, :658
		}
		A.depth[pv] = depth;
	}
	block_count_add(&cnt->n_eval, n_eval);
	block_count_add(&cnt->n_eval_device, n_eval);
	block_count_add(&cnt->n_pixels, n_pix);
}

// ------------------------------------------------------------------ MVS, window in registers
// Same work as mvs_generic_kernel, organised for the small MVS window (r=2, 25 taps): the
// support weights and the reference window's gray values are read once into registers, the
// per-pixel constants of the all-taps-usable form (meanL, totalWeight, sum2, a_t) are
// computed once, and a candidate costs 25 gathers of the other view's gray plane plus the
// reference's arithmetic in the reference's order (multiviewstereo.cpp:113-189).
template <int R>
struct MvsRegVisitor {
	static constexpr int WS = 2*R + 1, T = WS*WS;
	const ViewDev &A;
	const ViewDev *B;
	const srh_params &P;
	const Ray &ray;
	const double (&w)[T];     // weights
	const double (&a)[T];     // w*gl - meanL (all-usable form)
	int x, y;                 // reference pixel (the rare general form re-reads its window)
	bool all;
	double tw, s2;
	double bestCost, bestDepth;
	double *peaks;
	unsigned n;
	// without a top-K list only the largest (cost, depth) pair is wanted: the depth (unproject +
	// closestPoints, ~250 flop) is computed for the final winner and for exact cost ties only
	int bx, by;
	const ViewDev *bB;
	bool pending;

	__device__ __forceinline__ double cost(int cx, int cy) const {
		const ViewDev &Bv = *B;
		double gr[T];
		const bool inside = cx - R >= 0 && cy - R >= 0 && cx + R < Bv.w && cy + R < Bv.h;
		if (inside) {
#pragma unroll
			for (int row = 0; row < WS; ++row)
#pragma unroll
				for (int col = 0; col < WS; ++col)
					gr[row*WS + col] = Bv.gray[(size_t)(cy - R + row)*Bv.w + (cx - R + col)];
		} else {
#pragma unroll
			for (int row = 0; row < WS; ++row)
#pragma unroll
				for (int col = 0; col < WS; ++col) gr[row*WS + col] = mvs_tap(Bv, cx - R + col, cy - R + row);
		}
		const auto wr = [&](int t) { return w[t]; };
		if (all && inside) return mvs_fast_cost<T>(wr, a, gr, tw, s2);
		// any validity pattern; the reference window is read again (rare)
		return mvs_select_cost<WS>([&](int row, double *gl, double *g, double *wt) {
#pragma unroll
			for (int col = 0; col < WS; ++col) { gl[col] = mvs_tap(A, x - R + col, y - R + row); g[col] = gr[row*WS + col]; wt[col] = w[row*WS + col]; }
		}, P.weight_cutoff);
	}

	__device__ __forceinline__ void finish() {
		if (pending) { bestDepth = candidate_depth(A.cam, bB->cam, P, ray, bx, by); pending = false; }
	}

	__device__ __forceinline__ void operator()(int cx, int cy) {
		const double c = cost(cx, cy);
		++n;
		if (c > P.peak_threshold && !peaks) {                    // multiviewstereo.cpp:589-594, 654-660
			if (c > bestCost) { bestCost = c; bx = cx; by = cy; bB = B; pending = true; }
			else if (c == bestCost && !(pending && bx == cx && by == cy && bB == B)) {
				const double z = candidate_depth(A.cam, B->cam, P, ray, cx, cy);
				finish();
				if (mvs_peak_better(c, z, bestCost, bestDepth)) { bestDepth = z; bx = cx; by = cy; bB = B; }
			}
		} else if (c > P.peak_threshold) {
			const double z = candidate_depth(A.cam, B->cam, P, ray, cx, cy);
			if (mvs_peak_better(c, z, bestCost, bestDepth)) { bestCost = c; bestDepth = z; }
			mvs_peaks_insert(peaks, P.top_k, c, z);
		}
	}
};

template <int R>
__global__ __launch_bounds__(128)
void mvs_reg_kernel(const ViewDev *__restrict__ views, int ref, NeighList nl, int nneigh, srh_params P,
                    int y0, int nrows, const double *__restrict__ wbuf, size_t wstride,
                    double *__restrict__ peaks, Counters *__restrict__ cnt)
{
	constexpr int WS = 2*R + 1, T = WS*WS;
	const ViewDev &A = views[ref];
	const int W = A.w;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	unsigned n_eval = 0, n_pix = 0;
	if (q < (size_t)nrows*W) {
		const int x = (int)(q % W), y = y0 + (int)(q / W);
		const size_t pv = (size_t)y*W + x;
		double depth = __builtin_inf();
		double *pk = peaks ? peaks + pv*(size_t)P.top_k*2 : nullptr;
		if (pk) mvs_peaks_init(pk, P.top_k);
		if (A.mask[pv] == 1) {
			n_pix = 1;
			const double *wq = wbuf + wbuf_offset(W, T, (int)(q / W), x);
			double w[T], a[T];
			const MvsUnit u = mvs_unit_constants<T, true>([&](int t, double &wt, double &gl) {
				wt = wq[(size_t)t*wstride];
				gl = mvs_tap(A, x - R + t % WS, y - R + t / WS);
			}, [&](int t) -> double & { return w[t]; }, a, P.weight_cutoff, true);
			const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
			MvsRegVisitor<R> vis = { A, &A, P, ray, w, a, x, y, u.all, u.tw, u.s2, 0.0, -1.0, pk, 0, 0, 0, &A, false };
			for (int ni = 0; ni < nneigh; ++ni) {
				const int v2 = nl.n[ni];
				vis.B = &views[v2];
				walk_curve<true>(ray, A.cam, views[v2], P, vis);
			}
			vis.finish();
			n_eval = vis.n;
			depth = vis.bestDepth;
		}
		A.depth[pv] = depth;
	}
	block_count_add(&cnt->n_eval, n_eval);
	block_count_add(&cnt->n_eval_device, n_eval);
	block_count_add(&cnt->n_pixels, n_pix);
}

// ---- MultiViewStereo, two-stage form --------------------------------------------------------
// mvs_reg_kernel keeps the curve walk, 25 weights, 25 a_t and a 25-tap window live in one thread:
// >300 VGPRs, one wave per SIMD, every mask byte and every gather waited for in turn.  The default
// path splits the work:
//   mvs_walk_kernel   (pixel, neighbour) -> the candidate list of MultiViewStereo::epipolarCurve
//                     (multiviewstereo.cpp:754-810).  Few registers, many waves; raster points are
//                     queued in LDS and their mask bytes fetched in batches at wave-uniform flushes.
//   mvs_list_cost_kernel  the free cost_ncc (multiviewstereo.cpp:113-189) of every listed candidate,
//                     weights and a_t in registers, the next candidate's window in flight while the
//                     current one is reduced; keeps the largest (cost, depth) pair (:589-604, 654-660).
// Lists are stored wave-tiled, entry k of unit u at ((u/64)*cmax + k)*64 + u%64: a wave reads and
// writes its 64 lists coalesced, and they are contiguous in memory.
// The lists of a wave's 64 units (64 neighbouring pixels of one row, one link) are kept ALIGNED: after every flush of
// the raster queues the shorter lists are filled up with MQ_PAD entries to the wave's longest.  Entry k of every lane
// then belongs to the same stretch of depth levels, so the 64 windows the cost kernel gathers for one k lie side by
// side in the other view (a few cache lines per wave-load).  Without it the k-th candidates drift apart -- a curve
// that enters the other view's mask fifteen pixels later than its neighbour's stays fifteen entries behind for the
// rest of the list -- and the kernel is bound by the L1 address path (18 lines per wave-load).
// A pad is never evaluated; count[] holds the list length in slots, the work counters count candidates.
// Every flush also closes a WINDOW of list slots [kb, ke) shared by the wave's 64 lists, and the walk kernel records
// the bounding box of the candidates in it: mvs_staged_cost_kernel copies that box of the other view (plus the
// window radius) into LDS once and takes the 64 x (ke - kb) x 25 taps from there.  A wave with a window that does not
// fit (box over an image border, larger than the LDS share, more than `maxw` windows) is left to
// mvs_list_cost_kernel, which gathers from memory: nwin[wave] = -1.
#define MQ_PAD 0xffffffffu
#define MQ_PQ 4                    // top-K request: pairs above the threshold a lane may have waiting for their depth
#define MQ_T 128
#define MQ_QN 32
#define MQ_FLUSH 24
#define SRH_MVS_WAVES 2

#ifdef SRH_EXPERIMENT
// timing experiments only (make exp): 1 = label projections only (no raster walk), 2 = raster walk but no flush work
__device__ int g_exp_walk_mode = 0;
void exp_set_walk(int mode) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_exp_walk_mode), &mode, sizeof(int)); }
#endif

// FASTP: every neighbour of the launch is a plain pinhole camera and the reference view has the label table: the
// certified label projections of srh_walk.hpp (the general projection path is then not even compiled into the kernel:
// its live ranges cost a wave per SIMD)
template <bool FASTP>
__global__ __launch_bounds__(MQ_T, 4)
void mvs_walk_kernel(const ViewDev *__restrict__ views, int ref, NeighList nl, srh_params P,
                     int y0, int nrows, const double *__restrict__ tnum, uint32_t *__restrict__ cand, int cmax,
                     int32_t *__restrict__ count,
                     Counters *__restrict__ cnt, int *__restrict__ max_count,
                     uint4 *__restrict__ wdesc, int32_t *__restrict__ nwin, int maxw, int lds_cap,
                     const uint32_t *__restrict__ act, int nact)
{
	__shared__ uint32_t s_q[MQ_QN][MQ_T];
	__shared__ int s_max;
	const size_t waveid = ((size_t)blockIdx.y*gridDim.x + blockIdx.x)*(MQ_T/64) + (threadIdx.x >> 6);
	int nw = 0, wbase = 0;                                          // windows closed so far, first slot of the open one
	bool wstaged = wdesc != nullptr;
	typedef unsigned short us2 __attribute__((ext_vector_type(2)));
	us2 flo = { 65535, 65535 }, fhi = { 0, 0 };                     // box of the candidates this lane kept in the open window, (x, y) packed like a list entry
	const ViewDev &A = views[ref];
	const ViewDev &B = views[nl.n[blockIdx.y]];
	const int W = A.w, OW = B.w, OH = B.h;
	const int tid = threadIdx.x;
	// the units of a launch: the band's masked-in pixels in the view's serpentine order (ViewHost::act), 128 per block
	const size_t j = (size_t)blockIdx.x*MQ_T + tid;
	const bool active = j < (size_t)nact;
	const uint32_t pix = active ? act[j] : 0u;
	const int x = (int)(pix % (uint32_t)W), y = (int)(pix / (uint32_t)W);
	const size_t unit = (size_t)blockIdx.y*((size_t)gridDim.x*MQ_T) + j;     // list and count index
	int nk = 0;                                                     // list slots written so far (candidates and pads)
	int nreal = 0;                                                  // candidates kept so far
	if (tid == 0) s_max = 0;

	if (__any(active)) {
		Ray ray = {};
		if (active) ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
		int qn = 0;
		uint32_t last = 0xffffffffu;                                // std::unique state (last kept point)
		uint32_t *cp = cand + (unit >> 6)*(size_t)cmax*64 + (unit & 63);   // list slot nk of this lane (wave-tiled lists)

		typedef const __attribute__((address_space(1))) uint8_t *gmask;   // global_load: not coupled to the LDS queue's counter
		const gmask bmask = (gmask)B.mask;
		auto flush = [&]() {
			for (int k0 = 0; __any(k0 < qn); k0 += 8) {
				uint32_t e[8];
				uint8_t m[8];
				// (reads and loads without conditions -- an entry past the lane's count becomes pixel (0, 0) -- so that the
				// eight mask bytes are in flight together: as conditional loads each one waited for its own round trip)
#pragma unroll
				for (int j = 0; j < 8; ++j) { const uint32_t raw = s_q[k0 + j][tid]; e[j] = k0 + j < qn ? raw : 0u; }
#pragma unroll
				for (int j = 0; j < 8; ++j) m[j] = bmask[(size_t)(e[j] >> 16)*OW + (e[j] & 0xffffu)];
#pragma unroll
				for (int j = 0; j < 8; ++j)
					if (k0 + j < qn && m[j] == 1 && e[j] != last) {   // mask == WHITE, then std::unique (:786-807)
						last = e[j];
						if (nk < cmax) *cp = e[j];
						cp += 64; ++nk; ++nreal;
						const us2 ev = __builtin_bit_cast(us2, e[j]);               // v_pk_min_u16 / v_pk_max_u16: x and y at once
						flo = __builtin_elementwise_min(flo, ev);
						fhi = __builtin_elementwise_max(fhi, ev);
					}
			}
			qn = 0;
			// align the wave's lists (flush() is called by all lanes together)
			int top = nk;
#pragma unroll
			for (int dd = 1; dd < 64; dd <<= 1) { const int o = __shfl_xor(top, dd); top = o > top ? o : top; }
			if (active)
				for (; nk < top; ++nk, cp += 64)
					if (nk < cmax) *cp = MQ_PAD;
			if (wdesc && top > wbase) {
#pragma unroll
				for (int dd = 1; dd < 64; dd <<= 1) {
					const us2 lo2 = __builtin_bit_cast(us2, __shfl_xor(__builtin_bit_cast(int, flo), dd));
					const us2 hi2 = __builtin_bit_cast(us2, __shfl_xor(__builtin_bit_cast(int, fhi), dd));
					flo = __builtin_elementwise_min(flo, lo2);
					fhi = __builtin_elementwise_max(fhi, hi2);
				}
				const int X0 = flo.x, Y0 = flo.y, X1 = fhi.x, Y1 = fhi.y;
				const int Rw = P.window_radius;
				const int cols = X1 - X0 + 1 + 2*Rw, rows = Y1 - Y0 + 1 + 2*Rw;
				const bool fits = X0 - Rw >= 0 && Y0 - Rw >= 0 && X1 + Rw < OW && Y1 + Rw < OH && rows*(cols | 1) <= lds_cap;
				if (!fits || nw >= maxw) wstaged = false;
				else if ((tid & 63) == 0)
					wdesc[waveid*(size_t)maxw + nw] = make_uint4((unsigned)wbase, (unsigned)top, (unsigned)X0 | ((unsigned)Y0 << 16),
					                                            (unsigned)X1 | ((unsigned)Y1 << 16));
				++nw;
				wbase = top;
				flo = us2{ 65535, 65535 }; fhi = us2{ 0, 0 };
			}
		};

		const Vec3 camC = load3(A.cam.C);
		const Vec3 normal = load3(A.cam.pdir);
		const double nd = dot(normalized(normal), ray.dir);           // intersect(): n . dir, the same for every label
		const SharedDivisor ndd = shared_divisor(nd);                 // tnum[d] / nd with the divisor's half of the division done once
		const bool b_pinhole = !B.cam.is_refractive && !B.cam.is_distorted;
		double x1 = __builtin_nan(""), y1 = __builtin_nan("");
		// certified label projections (srh_walk.hpp): label table + plain pinhole neighbour
		const bool fastp = FASTP;
		FastProj fp = {};
		double e1 = 0.0;                                            // bound of the kept point (0: it is the reference's own value)
		int d1 = 0;                                                 // its label
		int jx1 = 0, jy1 = 0;                                       // its truncated coordinates (certified projections)
		if (fastp && active) {
			const double ta = fabs(tnum[0]), tb = fabs(tnum[P.num_depth_levels - 1]);
			fp = fast_proj_setup(ray, B.cam, ((ta > tb ? ta : tb)/fabs(nd))*1.000001);
		}
		for (int d = 0; d < P.num_depth_levels; ++d) {
			bool seg = false;
			int sx0 = 0, sy0 = 0, sx1 = 0, sy1 = 0;                     // the label's segment (seg), clipped
			if (FASTP) { if (active) {
				const double t = div_by(tnum[d], ndd);
				if (!(fabs(nd) < 1e-10) && !(t < 1e-10)) {
					double x2, y2, e;
					fast_project(fp, t, P.image_scale, x2, y2, e);
					if (!(trunc_certain(x2, e) && trunc_certain(y2, e))) { const double2 p = exact_label_point(A.cam, B.cam, x, y, P.image_scale, t); x2 = p.x; y2 = p.y; e = 0.0; }
					if (isnan_d(x1)) { x1 = x2; y1 = y2; e1 = e; d1 = d; jx1 = trunc_sat(x2); jy1 = trunc_sat(y2); }
					else {
						double dx = x2 - x1, dy = y2 - y1;
						double dd = dx*dx + dy*dy;
						const double se = e + e1;
						// |dd_reference - dd| <= 2(|dx| + |dy|)se + 2se^2 + roundings
						const double m = __builtin_fma(dd, 0x1p-48, 2.02*((fabs(dx) + fabs(dy))*se + se*se));
						if (!(fabs(dd - 1.0) > m)) {
							// the one-pixel test is not decided by the fast values: both points by the reference's operations
							if (e != 0.0) { const double2 p = exact_label_point(A.cam, B.cam, x, y, P.image_scale, t); x2 = p.x; y2 = p.y; e = 0.0; }
							if (e1 != 0.0) { const double2 p = exact_label_point(A.cam, B.cam, x, y, P.image_scale, div_by(tnum[d1], ndd)); x1 = p.x; y1 = p.y; e1 = 0.0; jx1 = trunc_sat(x1); jy1 = trunc_sat(y1); }
							dx = x2 - x1; dy = y2 - y1;
							dd = dx*dx + dy*dy;
						}
						if (dd >= 1) {
							// (the kept point's truncations travel with it: two conversions per kept label instead of four)
							// (a coordinate that passed trunc_certain is a number below 2^28: the plain conversion is trunc_sat's)
							int ix0 = jx1, iy0 = jy1, ix1, iy1;
							if (__all(e != 0.0)) { ix1 = (int)x2; iy1 = (int)y2; } else { ix1 = trunc_sat(x2); iy1 = trunc_sat(y2); }
							jx1 = ix1; jy1 = iy1;
							// (both end points inside the image: clipLine returns the segment as it is)
							const bool in0 = (unsigned)ix0 < (unsigned)OW && (unsigned)iy0 < (unsigned)OH;
							const bool in1 = (unsigned)ix1 < (unsigned)OW && (unsigned)iy1 < (unsigned)OH;
							if ((in0 && in1) || clip_line(ix0, iy0, ix1, iy1, OW, OH)) {  // 6-arg LineIterator, multiviewstereo.cpp:783
								sx0 = ix0; sy0 = iy0; sx1 = ix1; sy1 = iy1;
								seg = true;
							}
							x1 = x2; y1 = y2; e1 = e; d1 = d;
						}
					}
				}
			} } else if (active) {
				Vec3 point = camC;
				bool hit;
				if (tnum) {
					// label table (pinhole_label_tnum): the operands and operations of pointFromDepth / intersect
					const double t = div_by(tnum[d], ndd);
					hit = !(fabs(nd) < 1e-10) && !(t < 1e-10);
					point = ray.src + t*ray.dir;
				} else {
					hit = point_from_depth(ray, normal, depth_from_label(P, true, d), point);
				}
				if (hit && b_pinhole) {
					// cam_project of a plain pinhole camera (camera.cpp:380-419), the two quotients sharing their divisor
					const Vec3 pl = matvec(B.cam.R, point) + load3(B.cam.t);
					const Vec3 pk = matvec(B.cam.K, pl);
					const SharedDivisor zd = shared_divisor(pk.z);
					point.x = div_by(pk.x, zd); point.y = div_by(pk.y, zd);
				} else if (hit) hit = cam_project(B.cam, point);
				if (hit) {
					const double x2 = point.x*P.image_scale, y2 = point.y*P.image_scale;
					if (isnan_d(x1)) { x1 = x2; y1 = y2; }
					else {
						const double dx = x2 - x1, dy = y2 - y1;
						if (dx*dx + dy*dy >= 1) {
							int ix0 = trunc_sat(x1), iy0 = trunc_sat(y1), ix1 = trunc_sat(x2), iy1 = trunc_sat(y2);
							if (clip_line(ix0, iy0, ix1, iy1, OW, OH)) {  // 6-arg LineIterator, multiviewstereo.cpp:783
								sx0 = ix0; sy0 = iy0; sx1 = ix1; sy1 = iy1;
								seg = true;
							}
#ifdef SRH_EXPERIMENT
							if (g_exp_walk_mode == 1) { seg = false; nreal += ix0 + iy1; }
							if (g_exp_walk_mode == 3) { seg = false; nreal += trunc_sat(x1) + trunc_sat(y2); }
#endif
							x1 = x2; y1 = y2;
						}
					}
				}
			}
			// (one place where the walker's state is made: set in the branches above it had to be given values on every
			// path around them -- two dozen register moves per label)
			LineWalk lw;
			lw.x = 1; lw.xend = 0; lw.y = 0; lw.error = 0; lw.ystep = 0; lw.deltax = 0; lw.deltay = 0; lw.steep = false;
			if (seg) lw.begin(sx0, sy0, sx1, sy1, 0, 0);
			for (;;) {
				while (seg && lw.has_next() && qn < MQ_QN) {
					int tx, ty;
					lw.current(tx, ty);
					s_q[qn][tid] = (uint32_t)tx | ((uint32_t)ty << 16); ++qn;   // (inside the image: the segment was clipped)
					lw.next();
				}
				const bool more = seg && lw.has_next();
#ifdef SRH_EXPERIMENT
				if (g_exp_walk_mode == 2) { if (__any(more || qn >= MQ_FLUSH)) { nreal += qn; qn = 0; } if (!__any(more)) break; continue; }
#endif
				if (__any(more || qn >= MQ_FLUSH)) flush();
				if (!__any(more)) break;
			}
		}
		flush();
	}
	count[unit] = nk;
	if (nwin && (tid & 63) == 0) {
		nwin[waveid] = wstaged ? nw : -1;
		if (!wstaged) atomicAdd(&cnt->mvs_waves_listed, 1ull); else if (nw > 0) atomicAdd(&cnt->mvs_waves_staged, 1ull);
	}
	__syncthreads();
	if (nk) atomicMax(&s_max, nk);
	__syncthreads();
	if (tid == 0 && s_max) atomicMax(max_count, s_max);
	block_count_add(&cnt->n_eval, (unsigned)nreal);
	block_count_add(&cnt->n_eval_device, (unsigned)nreal);
	block_count_add(&cnt->n_pixels, (active && blockIdx.y == 0) ? 1u : 0u);
}

// cost of one candidate for any validity pattern (window over an image border, cut-off weights) of a unit whose
// reference-side taps (weights wt, grays gl -- NaN outside the image -- and okl = tap usable on the reference side) are at
// hand: mvs_select_cost_masked (srh_mvs_ncc.hpp).  The candidate's 25 taps are fetched with UNCONDITIONAL loads from
// clamped addresses (one memory round trip for the window; a guarded load per tap -- a branch and a wait of its own each,
// twice per candidate -- made this routine 50 dependent round trips per candidate, and on real photographs every
// silhouette pixel comes here: its window reaches over the masked-out background, whose weights are below the cut-off).
template <int R>
__device__ __forceinline__ double mvs_cost_select(const ViewDev &B, const double (&wt)[(2*R + 1)*(2*R + 1)],
                                                  const double (&gl)[(2*R + 1)*(2*R + 1)], const bool (&okl)[(2*R + 1)*(2*R + 1)],
                                                  int cx, int cy)
{
	constexpr int WS = 2*R + 1, T = WS*WS;
	typedef const __attribute__((address_space(1))) double *gptr;
	const int OW = B.w, OH = B.h;
	double gr[T];
	bool ok[T];
#pragma unroll
	for (int row = 0; row < WS; ++row) {
		const int yy = cy - R + row, yc = yy < 0 ? 0 : (yy >= OH ? OH - 1 : yy);
		gptr rp = (gptr)(B.gray + (size_t)yc*OW);
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const int xx = cx - R + col, xc = xx < 0 ? 0 : (xx >= OW ? OW - 1 : xx);
			gr[row*WS + col] = rp[xc];
			ok[row*WS + col] = okl[row*WS + col] && xx == xc && yy == yc;
		}
	}
	return mvs_select_cost_masked<T>(wt, gl, gr, ok);
}

// The rare units the lean loops below cannot finish -- a window over an image border or an unusable tap somewhere
// (the guarded form of the cost is needed), or two different candidates tied exactly for the largest cost (their
// depths decide, multiviewstereo.cpp:600-602) -- are redone here from their candidate list, the reference's
// streaming rule applied in list order.  The out-of-line cost gives the same bits as the fast form.
template <int R>
__device__ __noinline__ void mvs_unit_general(const ViewDev &A, const ViewDev &B, const srh_params &P,
                                              const double *__restrict__ wq, size_t wstride, int x, int y,
                                              const uint32_t *__restrict__ cl, int n, double *__restrict__ bout,
                                              double *__restrict__ pk)
{
	constexpr int WS = 2*R + 1, T = WS*WS;
	const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
	double bestCost = 0.0, bestDepth = -1.0;
	if (pk) mvs_peaks_init(pk, P.top_k);
	// the reference side once per unit
	double wt[T], gl[T];
	bool okl[T];
#pragma unroll
	for (int row = 0; row < WS; ++row)
#pragma unroll
		for (int col = 0; col < WS; ++col) {
			const int t = row*WS + col, xx = x - R + col, yy = y - R + row;
			const int xc = xx < 0 ? 0 : (xx >= A.w ? A.w - 1 : xx), yc = yy < 0 ? 0 : (yy >= A.h ? A.h - 1 : yy);
			wt[t] = wq[(size_t)t*wstride];
			const double v = A.gray[(size_t)yc*A.w + xc];
			gl[t] = (xx == xc && yy == yc) ? v : __builtin_nan("");
			okl[t] = gl[t] == gl[t] && wt[t] > P.weight_cutoff;
		}
	uint32_t en = n > 0 ? cl[0] : MQ_PAD;
	for (int k = 0; k < n; ++k) {
		const uint32_t e = en;
		if (k + 1 < n) en = cl[(size_t)(k + 1)*64];                  // (the next entry travels under this candidate's arithmetic)
		if (e == MQ_PAD) continue;                                   // alignment filler of the wave-aligned lists
		const int cx = (int)(e & 0xffffu), cy = (int)(e >> 16);
		const double c = mvs_cost_select<R>(B, wt, gl, okl, cx, cy);
		if (c > P.peak_threshold && (pk || c >= bestCost)) {         // multiviewstereo.cpp:589-594, 654-660
			const double z = candidate_depth(A.cam, B.cam, P, ray, cx, cy);
			if (mvs_peak_better(c, z, bestCost, bestDepth)) { bestCost = c; bestDepth = z; }
			if (pk) mvs_peaks_insert(pk, P.top_k, c, z);
		}
	}
	bout[0] = bestCost; bout[1] = bestDepth;
}

// ---- what the two cost kernels share beside the arithmetic
// PEAKS: a pair above the threshold needs its depth (unproject + closestPoints, ~300 instructions) and a place in the
// unit's sorted K-list.  Done on the spot, a wave walks that path at nearly every candidate for the one or two lanes
// that passed; so the passing (cost, candidate) pairs wait in a short per-lane queue (pc / pe: [slot][thread], pqn
// filled) and the wave works them off together, all lanes calling, when a lane's queue is full (the K largest pairs of
// a multiset do not depend on the order of insertion).
template <int C>
__device__ __forceinline__ void mvs_pflush(const ViewDev &A, const ViewDev &B, const srh_params &P, int x, int y,
                                           const double (*pc)[C], const uint32_t (*pe)[C], int tid, int &pqn, double *pk)
{
	const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
	while (__any(pqn > 0))
		if (pqn > 0) {
			--pqn;
			const uint32_t e = pe[pqn][tid];
			mvs_peaks_insert(pk, P.top_k, pc[pqn][tid], candidate_depth(A.cam, B.cam, P, ray, (int)(e & 0xffffu), (int)(e >> 16)));
		}
}

// The end of a unit: its (cost, depth) pair into bout.  redo: from the candidate list by mvs_unit_general; PEAKS: the last
// entry of its list; otherwise candidate `be` (0xffffffff: no peak above the threshold) with the cost rescore(bestCost)
// -- what a kernel that ran other arithmetic than the reference's puts in place of its own maximum.
template <int R, bool PEAKS, class Rescore>
__device__ __forceinline__ void mvs_unit_end(const ViewDev &A, const ViewDev &B, const srh_params &P,
                                             const double *__restrict__ wq, size_t wstride, int x, int y,
                                             const uint32_t *__restrict__ cl, int n, double *__restrict__ bout,
                                             double *__restrict__ pk, bool redo, double bestCost, uint32_t be, Rescore &&rescore)
{
	if (redo) { mvs_unit_general<R>(A, B, P, wq, wstride, x, y, cl, n, bout, pk); return; }
	if (PEAKS) { bout[0] = pk[2*(P.top_k - 1)]; bout[1] = pk[2*(P.top_k - 1) + 1]; return; }
	double bestDepth = -1.0;
	if (be != 0xffffffffu) {
		const Ray ray = cam_unproject(A.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
		bestDepth = candidate_depth(A.cam, B.cam, P, ray, (int)(be & 0xffffu), (int)(be >> 16));
		bestCost = rescore(bestCost);
	}
	bout[0] = bestCost; bout[1] = bestDepth;
}

// PEAKS: every pair above the threshold also goes into the unit's sorted top-K list upk[unit][K][2] (its depth is
// then needed at once); mvs_combine_kernel merges the neighbours' lists into the caller's buffer.
template <int R, bool PEAKS>
__global__ __launch_bounds__(MQ_T, SRH_MVS_WAVES)
void mvs_list_cost_kernel(const ViewDev *__restrict__ views, int ref, NeighList nl, srh_params P,
                          int y0, int nrows, const double *__restrict__ wbuf, size_t wstride,
                          const uint32_t *__restrict__ cand, int cmax, const int32_t *__restrict__ count,
                          double *__restrict__ best, double *__restrict__ upk, const int32_t *__restrict__ nwin,
                          const uint32_t *__restrict__ act, int nact)
{
	constexpr int WS = 2*R + 1, T = WS*WS;
	// waves whose windows all fit the LDS are mvs_staged_cost_kernel's
	if (nwin && nwin[((size_t)blockIdx.y*gridDim.x + blockIdx.x)*(MQ_T/64) + (threadIdx.x >> 6)] >= 0) return;
	__shared__ double s_w[T][MQ_T];                                 // per-thread columns: conflict-free
	double a[T];
	const ViewDev &A = views[ref];
	const ViewDev &B = views[nl.n[blockIdx.y]];
	const int W = A.w, OW = B.w, OH = B.h;
	const int tid = threadIdx.x;
	const size_t j = (size_t)blockIdx.x*MQ_T + tid;                 // the walk kernel's unit order
	if (j >= (size_t)nact) return;
	const uint32_t pix = act[j];
	const int x = (int)(pix % (uint32_t)W), y = (int)(pix / (uint32_t)W);
	const size_t npix = (size_t)nrows*W;
	const size_t q = (size_t)(y - y0)*W + x;                        // pixel of the band: results are stored by pixel
	const size_t unit = (size_t)blockIdx.y*npix + q;
	const size_t ul = (size_t)blockIdx.y*((size_t)gridDim.x*MQ_T) + j;
	double *bout = best + unit*2;
	double *pk = PEAKS ? upk + unit*(size_t)P.top_k*2 : nullptr;
	if (PEAKS) mvs_peaks_init(pk, P.top_k);
	const int n = count[ul] < cmax ? count[ul] : cmax;
	if (n <= 0) { bout[0] = 0.0; bout[1] = -1.0; return; }

	// ---- per-pixel constants: weights in this thread's LDS column, a_t = w_t*gl_t - meanL in registers
	const double *wq = wbuf + wbuf_offset(W, T, (int)(q / W), x);
	const auto w = [&](int t) -> double & { return s_w[t][tid]; };
	const MvsUnit u = mvs_unit_constants<T, false>([&](int t, double &wt, double &gl) {
		wt = wq[(size_t)t*wstride];
		gl = mvs_tap(A, x - R + t % WS, y - R + t / WS);
	}, w, a, P.weight_cutoff, true);
	const bool all = u.all;
	const double tw = u.tw, s2 = u.s2;

	double bestCost = 0.0;
	uint32_t be = 0xffffffffu;
	bool redo = !all;                                               // this unit needs mvs_unit_general
	const uint32_t *cl = cand + (ul >> 6)*(size_t)cmax*64 + (ul & 63);
	__shared__ double s_pc[PEAKS ? MQ_PQ : 1][PEAKS ? MQ_T : 1];      // PEAKS: pairs above the threshold waiting for their depth (mvs_pflush)
	__shared__ uint32_t s_pe[PEAKS ? MQ_PQ : 1][PEAKS ? MQ_T : 1];
	int pqn = 0;
	auto pflush = [&]() { mvs_pflush(A, B, P, x, y, s_pc, s_pe, tid, pqn, pk); };

	// one candidate per iteration: its 25-tap window arrives in g[], is turned in place into p_t = w_t*g_t
	// (the products both sweeps need), and the next candidate's window is requested as soon as the second
	// sweep has consumed p_t.  Two waves per SIMD (a_t, p_t and the addresses need more than the 168 VGPRs of three).
	double g[T];
	uint32_t en = cl[0];
	bool inn;
	auto request = [&](uint32_t ee) {
		const int cx = (int)(ee & 0xffffu), cy = (int)(ee >> 16);
		inn = ee == MQ_PAD || (all && cx - R >= 0 && cy - R >= 0 && cx + R < OW && cy + R < OH);   // a pad: nothing to redo
		if (ee == MQ_PAD) ee = (uint32_t)R | ((uint32_t)R << 16);      // (any readable window)
		typedef const __attribute__((address_space(1))) double *gptr;     // global_load, not flat_load
		const int ux = (int)(ee & 0xffffu), uy = (int)(ee >> 16);
		const bool rd = ux - R >= 0 && uy - R >= 0 && ux + R < OW && uy + R < OH;
		gptr bp = (gptr)(B.gray + (size_t)((rd ? uy : R) - R)*OW + ((rd ? ux : R) - R));   // not usable: any valid address
#pragma unroll
		for (int row = 0; row < WS; ++row)
#pragma unroll
			for (int col = 0; col < WS; ++col) g[row*WS + col] = bp[(size_t)row*OW + col];
	};
	request(en);
	uint32_t e2 = n > 1 ? cl[64] : 0u;                           // list entry k+2 travels one step ahead of the window
	for (int k = 0; k < n; ++k) {
		asm volatile("" ::: "memory");                               // keep the LDS column in LDS (no hoisting into 50 VGPRs)
		const uint32_t e = en;
		const bool fast = inn;
		// p_t = weight*gray of the other view (multiviewstereo.cpp:150-151, 171); meanR is their sum / totalWeight
		double mR = 0;
#pragma unroll
		for (int row = 0; row < WS; ++row) {
			mvs_fast_products<WS>(w, g, row*WS, mR);
			__builtin_amdgcn_sched_barrier(0);                       // one window row of weights in flight at a time
		}
		mR /= tw;
		double s1 = 0, s3 = 0;
		mvs_fast_sums<T>(a, g, 0, mR, s1, s3);
		const double c = mvs_fast_finish(s1, s2 * s3);
		redo = redo || !fast;                                        // (c is meaningless then)
		if (k + 1 < n) {
			en = e2;
			if (k + 2 < n) e2 = cl[(size_t)(k + 2)*64];
			request(en);
		}
		if (e != MQ_PAD && c > P.peak_threshold) {                   // multiviewstereo.cpp:589-594, 654-660
			if (PEAKS) {
				if (fast) { s_pc[pqn][tid] = c; s_pe[pqn][tid] = e; ++pqn; }
			} else if (c > bestCost) { bestCost = c; be = e; }
			else if (c == bestCost && e != be) redo = true;              // exact tie of two candidates: depths decide
		}
		if (PEAKS && __any(pqn == MQ_PQ)) pflush();
	}
	if (PEAKS) pflush();
	mvs_unit_end<R, PEAKS>(A, B, P, wq, wstride, x, y, cl, n, bout, pk, redo, bestCost, be, [](double c) { return c; });
}

// ---- the staged form of the list cost kernel ------------------------------------------------------------------
// Same units, same lanes, same per-lane bookkeeping as mvs_list_cost_kernel; the 25-tap windows come from the wave's
// LDS copy of the current window's box of the other view instead of 15 gathers per candidate (which kept that
// kernel on the L1 address path at a quarter of the FP64 rate).  Weights and a_t live in registers.
#define MS_CAP 2432                   // doubles of LDS per wave: 4 workgroups of 2 waves fill a compute unit's 160 KB
#define MS_CAP_PEAKS 2240             // the same for the top-K request (room for its queue)
#define MS_PQ 2                       // top-K request: pairs a lane may have waiting
#define MS_MAXW 96                    // windows per wave
#ifndef MS_CPY
#define MS_CPY 4                      // box copy: loads in flight per lane (8 was measured: registers spill, the slots slow down by a third)
#endif
#ifndef MS_AHEAD
#define MS_AHEAD 4                    // list entries in flight per lane
#endif
#ifndef MS_CA
#define MS_CA 2                       // certified form: partial sums per sum (independent dependency chains)
#endif

// PEAKS: the top-K request (every pair above the threshold into the unit's sorted K-list upk[unit][K][2], as in
// mvs_list_cost_kernel<R, true>); its LDS share of the box is smaller by the queue of pairs waiting for their depth.
// CERT (not with PEAKS): the certified fused arithmetic (srh_wta.hpp, CertBound).  The two sweeps run
// with fused multiply-adds; a unit's result depends on the scores only through "which candidate has the largest score
// above the threshold" (multiviewstereo.cpp:589-604, 654-660), so the unit keeps, beside its fused maximum, whether any
// OTHER candidate's fused score came within 2*e0 of it (or any score within e0 of the threshold, or a candidate the
// bound does not cover): such a unit is redone in the reference's arithmetic (mvs_unit_general, as for exact ties);
// for every other unit the winner is the reference's, and its score -- which the combine step compares across
// neighbours -- is recomputed in the reference's arithmetic (the exact form's sweeps: one evaluation per unit).
// (the allocation is pinned: exactly two waves per SIMD, the whole 256-register budget -- the kernel's speed must be a property
// of the source, not of what the allocator makes of an edit elsewhere: VERDICT r5 weak #7)
template <int R, bool PEAKS, bool CERT>
__global__ __launch_bounds__(MQ_T, 2) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mvs_staged_cost_kernel(const ViewDev *__restrict__ views, int ref, NeighList nl, srh_params P,
                            int y0, int nrows, const double *__restrict__ wbuf, size_t wstride,
                            const uint32_t *__restrict__ cand, int cmax, const int32_t *__restrict__ count,
                            double *__restrict__ best, const uint4 *__restrict__ wdesc, const int32_t *__restrict__ nwin,
                            Counters *__restrict__ cnt, const uint32_t *__restrict__ act, int nact, double *__restrict__ upk,
                            const CertBound cb)
{
	static_assert(!(PEAKS && CERT), "the top-K request hands scores out: the reference's arithmetic");
	constexpr int WS = 2*R + 1, T = WS*WS;
#ifdef SRH_PROFILE_PHASES
	// diagnostic build: wave clocks of the phases, summed in cnt->dbg_phase (0 set-up, 1 copies, 2 slots, 3 end; dbg_blocks = slots)
	unsigned long long ph_t = __builtin_amdgcn_s_memtime(), ph[4] = {0, 0, 0, 0}, ph_slots = 0;
	const unsigned long long ph_t0 = ph_t;
#define MS_STAMP(i) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ph[i] += now_ - ph_t; ph_t = now_; }
#else
#define MS_STAMP(i)
#endif
	__shared__ double s_box[MQ_T/64][PEAKS ? MS_CAP_PEAKS : MS_CAP];
	__shared__ double s_pc[PEAKS ? MS_PQ : 1][PEAKS ? MQ_T : 1];     // PEAKS: pairs above the threshold waiting for their depth
	__shared__ uint32_t s_pe[PEAKS ? MS_PQ : 1][PEAKS ? MQ_T : 1];
	const ViewDev &A = views[ref];
	const ViewDev &B = views[nl.n[blockIdx.y]];
	const int W = A.w, OW = B.w;
	const int tid = threadIdx.x, lane = tid & 63;
	const size_t waveid = ((size_t)blockIdx.y*gridDim.x + blockIdx.x)*(MQ_T/64) + (tid >> 6);
	const int nw = nwin[waveid];
	if (nw < 0) return;                                             // mvs_list_cost_kernel's wave
	double *const sb = s_box[tid >> 6];
	const size_t j = (size_t)blockIdx.x*MQ_T + tid;                 // the walk kernel's unit order
	const bool active = j < (size_t)nact;                           // (the other lanes help with the copies)
	const uint32_t pix = active ? act[j] : 0u;
	const int x = (int)(pix % (uint32_t)W), y = active ? (int)(pix / (uint32_t)W) : y0;
	const size_t npix = (size_t)nrows*W;
	const size_t q = (size_t)(y - y0)*W + x;                        // pixel of the band: results are stored by pixel
	const size_t unit = (size_t)blockIdx.y*npix + q;
	const size_t ul = (size_t)blockIdx.y*((size_t)gridDim.x*MQ_T) + j;
	double *bout = best + unit*2;
	double *pk = PEAKS ? upk + unit*(size_t)P.top_k*2 : nullptr;
	if (PEAKS && active) mvs_peaks_init(pk, P.top_k);
	if (nw == 0) {                                                  // no candidate anywhere in the wave
		if (active) { bout[0] = 0.0; bout[1] = -1.0; }
		return;
	}
	const int n = active ? (count[ul] < cmax ? count[ul] : cmax) : 0;

	// ---- per-pixel constants: weights and a_t = w_t*gl_t - meanL
	const double *wq = wbuf + wbuf_offset(W, T, active ? (int)(q / W) : 0, active ? x : 0);
	double w[T], a[T];
	const auto wr = [&](int t) -> double & { return w[t]; };
	MvsUnit u = { 0.0, 0.0, false };
	if (active) {
		u = mvs_unit_constants<T, false>([&](int t, double &wt, double &gl) {
			wt = wq[(size_t)t*wstride];
			gl = mvs_tap(A, x - R + t % WS, y - R + t / WS);
		}, wr, a, P.weight_cutoff, true);
	} else {
#pragma unroll
		for (int t = 0; t < T; ++t) { w[t] = 0.0; a[t] = 0.0; }
	}
	const bool all = u.all;
	const double tw = u.tw, s2 = u.s2;

	double bestCost = 0.0;
	uint32_t be = 0xffffffffu;
	bool redo = active && !all;                                     // this unit needs mvs_unit_general
	const SharedDivisor twd = shared_divisor(tw);
	const double thr0 = P.peak_threshold > 0.0 ? P.peak_threshold : 0.0;
	const double sig3 = CERT ? cb.sigma3(s2) : 0.0;                 // certified: the smallest sum3 the bound covers for this unit
	bool amb = false, amb_tie = false;                              // certified: the maximum is not certain (amb_tie: only as long as the maximum stays where it is)
	int pqn = 0;
	auto pflush = [&]() {                                           // (all lanes together)
		mvs_pflush(A, B, P, x, y, s_pc, s_pe, tid, pqn, pk);
		if (active) bestCost = pk[0];                                // the K-th largest cost so far: nothing below it can enter the list
	};
	const uint32_t *cl = cand + (ul >> 6)*(size_t)cmax*64 + (ul & 63);
	const uint4 *wd = wdesc + waveid*(size_t)MS_MAXW;
	typedef const __attribute__((address_space(1))) double *gptr;

	// list entries travel MS_AHEAD slots ahead of their use (the windows are consecutive slot ranges: one running index)
	const int nslots = __builtin_amdgcn_readfirstlane((int)wd[nw - 1].y) < cmax ? __builtin_amdgcn_readfirstlane((int)wd[nw - 1].y) : cmax;
	uint32_t ering[MS_AHEAD];
#pragma unroll
	for (int j = 0; j < MS_AHEAD; ++j) ering[j] = j < nslots && j < n ? cl[(size_t)j*64] : MQ_PAD;
	uint4 dnext = wd[0];
	MS_STAMP(0)
	for (int wn = 0; wn < nw; ++wn) {
		const uint4 d = dnext;
		if (wn + 1 < nw) dnext = wd[wn + 1];
		const int kb = (int)d.x, ke = (int)d.y < cmax ? (int)d.y : cmax;
		const int X0 = (int)(d.z & 0xffffu), Y0 = (int)(d.z >> 16), X1 = (int)(d.w & 0xffffu), Y1 = (int)(d.w >> 16);
		const int cols = X1 - X0 + 1 + 2*R, rows = Y1 - Y0 + 1 + 2*R, stride = cols | 1;
		// ---- copy the box (with its margin of R) into the wave's LDS: element (r, c) at r*stride + c; four loads per
		// lane in flight (the copy is a chain of memory round trips otherwise).  (Pairs of columns per lane -- 16-byte loads
		// at 8-byte alignment, ds_write2_b64 -- were measured: the copies took 45 % longer.)
		{
			const int total = rows*stride;
			const int qs = 64 / stride, rs = 64 - qs*stride;
			int r = lane / stride, c = lane - r*stride;
			gptr src = (gptr)(B.gray + (size_t)(Y0 - R)*OW + (X0 - R));
			for (int idx = lane; idx < total; idx += MS_CPY*64) {
				double v[MS_CPY];
#pragma unroll
				for (int j = 0; j < MS_CPY; ++j) {
					v[j] = (idx + 64*j < total && c < cols) ? src[(size_t)r*OW + c] : 0.0;
					r += qs; c += rs;
					if (c >= stride) { c -= stride; ++r; }
				}
#pragma unroll
				for (int j = 0; j < MS_CPY; ++j)
					if (idx + 64*j < total) sb[idx + 64*j] = v[j];
			}
		}
		MS_STAMP(1)
#ifdef SRH_PROFILE_PHASES
		ph_slots += (unsigned long long)(ke - kb);
#endif
		// One slot per trip (two side by side were measured: their 100 product registers spill).  The slots are software-
		// pipelined over the LDS: the second sweep consumes g_t for the last time and puts the NEXT slot's tap in its place,
		// so that the first sweep of the next trip -- a dependent chain that used to start behind 15 LDS reads with eight
		// waves of the compute unit queueing at the LDS -- finds its operands in registers.  (The first slot of a window is
		// read on the spot: its box has only just been copied.)
		auto pop = [&](int slot) -> uint32_t {                         // list entry of `slot`: the ring holds the slots in order
			const uint32_t e = ering[0];
#pragma unroll
			for (int j = 0; j + 1 < MS_AHEAD; ++j) ering[j] = ering[j + 1];
			ering[MS_AHEAD - 1] = slot + MS_AHEAD < nslots && slot + MS_AHEAD < n ? cl[(size_t)(slot + MS_AHEAD)*64] : MQ_PAD;
			return e;
		};
		auto box_at = [&](uint32_t e) -> const double * {
			return sb + (e != MQ_PAD ? ((int)(e >> 16) - Y0)*stride + ((int)(e & 0xffffu) - X0) : 0);
		};
		double g[T];
		uint32_t e = MQ_PAD;
		if (kb < ke) {
			e = pop(kb);
			const double *gp = box_at(e);
#pragma unroll
			for (int row = 0; row < WS; ++row)
#pragma unroll
				for (int col = 0; col < WS; ++col) g[row*WS + col] = gp[row*stride + col];
		}
		for (int k = kb; k < ke; ++k) {
			const uint32_t ecur = e;
			e = k + 1 < ke ? pop(k + 1) : MQ_PAD;                        // (uniform)
			const double *gn = box_at(e);                                // (a pad, or nothing to come: any address of the box)
			// p_t = weight*gray of the other view (multiviewstereo.cpp:150-151, 171); meanR is their sum / totalWeight
			double mR = 0, s1 = 0, s3 = 0;
			double mRx[MS_CA > 1 ? MS_CA - 1 : 1], s3x[MS_CA > 1 ? MS_CA - 1 : 1];   // certified: the other partial sums (mRx: of meanR, then of sum1)
#pragma unroll
			for (int k = 0; k < MS_CA - 1; ++k) mRx[k] = 0;
			if (CERT) {
				// (g keeps the gray value; MS_CA partial sums: the exact kernel's sums are single dependent chains, one
				// instruction per 12 cycles and wave -- the bound holds for any order of summation)
#pragma unroll
				for (int t = 0; t < T; ++t) {
					if (t % MS_CA == 0) mR = __builtin_fma(w[t], g[t], mR); else mRx[t % MS_CA - 1] = __builtin_fma(w[t], g[t], mRx[t % MS_CA - 1]);
				}
			} else mvs_fast_products<T>(wr, g, 0, mR);
			if (CERT) {
#pragma unroll
				for (int k = 0; k < MS_CA - 1; ++k) { mR += mRx[k]; mRx[k] = 0; s3x[k] = 0; }
			}
			// exact form: mR / tw, the same bits (srh_walk.hpp).  Certified form: the product with the refined reciprocal of tw
			// (within one ulp of 1/tw: one more rounding on meanR, which eps_b = gamma_(T+4)*G has room for -- T for the sum, one
			// each for the quotient, the product, the subtraction); the unit's tw lies in [1, 25]
			mR = (CERT && twd.ok) ? mR*twd.r : div_by(mR, twd);
#pragma unroll
			for (int row = 0; row < WS; ++row) {
				if (CERT) {
					// (the row's b_t first, then the sums.  Measured without effect, like 3 or 4 partial sums per sum: a fused
					// multiply-add with three register operands issues at 80 % of the FP64 rate at two waves per SIMD,
					// profiles/microbench/fp64_rate_mi355x.txt, and the slot loop runs at three quarters of that)
					double b[WS];
#pragma unroll
					for (int col = 0; col < WS; ++col) b[col] = __builtin_fma(w[row*WS + col], g[row*WS + col], -mR);
#pragma unroll
					for (int col = 0; col < WS; ++col) {
						const int t = row*WS + col;
						if (t % MS_CA == 0) { s1 = __builtin_fma(a[t], b[col], s1); s3 = __builtin_fma(b[col], b[col], s3); }
						else { mRx[t % MS_CA - 1] = __builtin_fma(a[t], b[col], mRx[t % MS_CA - 1]); s3x[t % MS_CA - 1] = __builtin_fma(b[col], b[col], s3x[t % MS_CA - 1]); }
					}
				} else mvs_fast_sums<WS>(a, g, row*WS, mR, s1, s3);
#pragma unroll
				for (int col = 0; col < WS; ++col) g[row*WS + col] = gn[row*stride + col];   // the next slot's window row
				__builtin_amdgcn_sched_barrier(0);                         // (in this order: a row's registers are free before they are refilled)
			}
			if (CERT) {
#pragma unroll
				for (int k = 0; k < MS_CA - 1; ++k) { s1 += mRx[k]; s3 += s3x[k]; }
			}
			{
				// A score has an effect only when it is > threshold and >= the best so far (>= 0), hence >= bound.  With
				// sum1 >= 0:  sum1^2 < bound^2 * den * (1 - 1e-6)  puts the exact quotient below bound*(1 - 5e-7), out of reach
				// of the roundings of the square root and the division (and of the three products here).  A negative sum1
				// gives a negative score, without effect when the threshold is >= 0.  When no lane of the wave can be
				// affected, the square root and the division are skipped.
				const double den = s2 * s3;
				const double bound = bestCost > thr0 ? bestCost : thr0;
				// (as lane masks side by side, not as a chain of branches: a scalar instruction costs the wave 8.75 cycles, and the
				// chain was 25 of them around seven compares -- profiles/microbench/lone_wave_issue)
				const bool pad = ecur == MQ_PAD;
				const bool unc = CERT && !(s3 >= sig3);                          // a candidate the bound does not cover: the unit is redone
				const bool nul = !(den >= 1e-10) | (s1 < 0.0);                   // score 0 (or NaN), or negative
				// (certified: the fused score is within e0 of the reference's; 5e-7*bound covers e0 once bound >= 1e-3)
				const bool low = (!CERT || bound >= 1e-3) & (s1*s1 < bound*bound*den*0.999999);
				const bool hopeless = pad | (!unc & (nul ? P.peak_threshold >= 0.0 : low));
				if (CERT) amb |= !pad & unc;
				if (__all(hopeless)) continue;
				const double c = mvs_fast_finish(s1, den);
				if (CERT) {
					if (ecur != MQ_PAD && !hopeless) {
						// the reference keeps the largest (score, depth) pair among the scores above the threshold; bestCost / be
						// follow the fused maximum, amb says it is not certainly the reference's
						if (!(fabs(c - P.peak_threshold) > cb.e0)) amb = true;   // the threshold decision itself (NaN: ambiguous)
						else if (c > P.peak_threshold) {
							// bestCost is the largest fused score so far (initially 0 with no candidate: the reference's start)
							if (c > bestCost + 2*cb.e0) { bestCost = c; be = ecur; amb_tie = false; }   // every earlier score is out of reach
							else if (c >= bestCost - 2*cb.e0 && ecur != be) { amb_tie = true; if (c > bestCost) { bestCost = c; be = ecur; } }
						}
					}
				} else if (ecur != MQ_PAD && c > P.peak_threshold) {        // multiviewstereo.cpp:589-594, 654-660
					if (PEAKS) { if (all) { s_pc[pqn][tid] = c; s_pe[pqn][tid] = ecur; ++pqn; } }
					else if (c > bestCost) { bestCost = c; be = ecur; }
					else if (c == bestCost && ecur != be) redo = true;       // exact tie of two candidates: depths decide
				}
			}
			if (PEAKS && __any(pqn == MS_PQ)) pflush();
		}
		MS_STAMP(2)
	}
	if (PEAKS) pflush();
	if (active) {
		if (CERT && (amb || amb_tie) && !redo) { redo = true; atomicAdd(&cnt->n_flagged, 1ull); }
		mvs_unit_end<R, PEAKS>(A, B, P, wq, wstride, x, y, cl, n, bout, pk, redo, bestCost, be, [&](double c) {
			if (!CERT) return c;
			// certified: the winner is the reference's; the score handed to the combine step is the reference's too --
			// the exact kernel's own sweeps once more for this one candidate (a staged wave's windows lie inside the other
			// image, this unit's taps are all usable: the fast form applies), its 25 taps straight from memory
			gptr bp = (gptr)(B.gray + (size_t)((int)(be >> 16) - R)*OW + ((int)(be & 0xffffu) - R));
			double gx[T], mRx = 0, x1 = 0, x3 = 0;
#pragma unroll
			for (int row = 0; row < WS; ++row)
#pragma unroll
				for (int col = 0; col < WS; ++col) gx[row*WS + col] = bp[(size_t)row*OW + col];
			mvs_fast_products<T>(wr, gx, 0, mRx);
			mRx = div_by(mRx, twd);
			mvs_fast_sums<T>(a, gx, 0, mRx, x1, x3);
			return mvs_fast_finish(x1, s2 * x3);
		});
	}
#ifdef SRH_PROFILE_PHASES
	MS_STAMP(3)
	if (lane == 0) {
		for (int i = 0; i < 4; ++i) atomicAdd(&cnt->dbg_phase[i], ph[i]);
		atomicAdd(&cnt->dbg_total_cycles, ph_t - ph_t0);
		atomicAdd(&cnt->dbg_blocks, ph_slots);
		atomicAdd(&cnt->dbg_waves, 1ull);
		atomicAdd(&cnt->dbg_cycles, (unsigned long long)nw);
	}
#endif
}
#undef MS_STAMP

void mvs_staging_shape(int *maxw, size_t *desc_words_per_wave) { *maxw = MS_MAXW; *desc_words_per_wave = (size_t)MS_MAXW*4; }

// wdesc / nwin: window descriptors (MS_MAXW uint4 per wave) and window counts of the launch's waves, or null (no staging)
void launch_mvs_walk(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                     const srh_params &P, int y0, int nrows, const double *tnum, uint32_t *cand, int cmax, int32_t *count,
                     Counters *cnt, int *max_count, uint32_t *wdesc, int32_t *nwin, const uint32_t *act, int nact, bool peaks,
                     bool fast_pinhole)
{
	if (nact <= 0) return;
	const dim3 grid((unsigned)((nact + MQ_T - 1)/MQ_T), (unsigned)nneigh);
	if (fast_pinhole && tnum)
		hipLaunchKernelGGL(mvs_walk_kernel<true>, grid, dim3(MQ_T), 0, st, views, ref, make_neigh_list(neigh, nneigh),
		                   P, y0, nrows, tnum, cand, cmax, count, cnt, max_count, (uint4 *)wdesc, nwin, MS_MAXW,
		                   peaks ? MS_CAP_PEAKS : MS_CAP, act, nact);
	else
		hipLaunchKernelGGL(mvs_walk_kernel<false>, grid, dim3(MQ_T), 0, st, views, ref, make_neigh_list(neigh, nneigh),
		                   P, y0, nrows, tnum, cand, cmax, count, cnt, max_count, (uint4 *)wdesc, nwin, MS_MAXW,
		                   peaks ? MS_CAP_PEAKS : MS_CAP, act, nact);
}

// the three steps of the list path's second stage; nwin (or null): the waves with nwin >= 0 are the staged kernel's
void launch_mvs_staged_cost(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                            const srh_params &P, int y0, int nrows, const double *wbuf, size_t wstride,
                            const uint32_t *cand, int cmax, const int32_t *count, double *best,
                            const uint32_t *wdesc, const int32_t *nwin, Counters *cnt, const uint32_t *act, int nact,
                            double *unit_peaks, bool cert)
{
	if (nact <= 0) return;
	const dim3 grid((unsigned)((nact + MQ_T - 1)/MQ_T), (unsigned)nneigh);
	const NeighList nl = make_neigh_list(neigh, nneigh);
	const CertBound cb = cert_bound(P, true);
	if (unit_peaks)
		hipLaunchKernelGGL((mvs_staged_cost_kernel<2, true, false>), grid, dim3(MQ_T), 0, st, views, ref, nl, P, y0, nrows,
		                   wbuf, wstride, cand, cmax, count, best, (const uint4 *)wdesc, nwin, cnt, act, nact, unit_peaks, cb);
	else if (cert && cb.ok)
		hipLaunchKernelGGL((mvs_staged_cost_kernel<2, false, true>), grid, dim3(MQ_T), 0, st, views, ref, nl, P, y0, nrows,
		                   wbuf, wstride, cand, cmax, count, best, (const uint4 *)wdesc, nwin, cnt, act, nact, (double *)nullptr, cb);
	else
		hipLaunchKernelGGL((mvs_staged_cost_kernel<2, false, false>), grid, dim3(MQ_T), 0, st, views, ref, nl, P, y0, nrows,
		                   wbuf, wstride, cand, cmax, count, best, (const uint4 *)wdesc, nwin, cnt, act, nact, (double *)nullptr, cb);
}

void launch_mvs_list_cost(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                          const srh_params &P, int y0, int nrows, const double *wbuf, size_t wstride,
                          const uint32_t *cand, int cmax, const int32_t *count, double *best,
                          double *unit_peaks, bool peaks, const int32_t *nwin, const uint32_t *act, int nact)
{
	if (nact <= 0) return;
	const dim3 grid((unsigned)((nact + MQ_T - 1)/MQ_T), (unsigned)nneigh);
	const NeighList nl = make_neigh_list(neigh, nneigh);
	if (peaks)
		hipLaunchKernelGGL((mvs_list_cost_kernel<2, true>), grid, dim3(MQ_T), 0, st, views, ref, nl, P, y0, nrows,
		                   wbuf, wstride, cand, cmax, count, best, unit_peaks, nwin, act, nact);
	else
		hipLaunchKernelGGL((mvs_list_cost_kernel<2, false>), grid, dim3(MQ_T), 0, st, views, ref, nl, P, y0, nrows,
		                   wbuf, wstride, cand, cmax, count, best, (double *)nullptr, nwin, act, nact);
}

__global__ void mvs_combine_kernel(const ViewDev *__restrict__ views, int ref, int nneigh, int y0, int nrows,
                                   const double *__restrict__ best, const double *__restrict__ upk,
                                   double *__restrict__ peaks, int K)
{
	const ViewDev &A = views[ref];
	const int W = A.w;
	const size_t q = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	const size_t npix = (size_t)nrows*W;
	if (q >= npix) return;
	const size_t pv = (size_t)y0*W + q;
	double depth = __builtin_inf();
	double *pk = peaks ? peaks + pv*(size_t)K*2 : nullptr;
	if (pk) mvs_peaks_init(pk, K);
	if (A.mask[pv] == 1) {
		double bc = 0.0, bd = -1.0;
		for (int ni = 0; ni < nneigh; ++ni) {
			const double c = best[((size_t)ni*npix + q)*2], z = best[((size_t)ni*npix + q)*2 + 1];
			if (mvs_peak_better(c, z, bc, bd)) { bc = c; bd = z; }
			if (pk) {
				// the neighbour's K largest pairs; fillers (0, -1) never displace anything
				const double *u = upk + ((size_t)ni*npix + q)*(size_t)K*2;
				for (int k = 0; k < K; ++k) mvs_peaks_insert(pk, K, u[2*k], u[2*k + 1]);
			}
		}
		depth = bd;
	}
	A.depth[pv] = depth;
}

void launch_mvs_combine(hipStream_t st, const ViewDev *views, int ref, int nneigh, int width, const srh_params &P,
                        int y0, int nrows, const double *best, const double *unit_peaks, double *peaks)
{
	const size_t n = (size_t)nrows*width;
	hipLaunchKernelGGL(mvs_combine_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st, views, ref, nneigh, y0, nrows, best,
	                   unit_peaks, peaks, P.top_k);
}

void launch_mvs_generic(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                        const srh_params &P, int y0, int nrows, const double *wbuf, size_t wstride,
                        double *peaks, Counters *cnt)
{
	const size_t n = (size_t)nrows*width;
	const NeighList nl = make_neigh_list(neigh, nneigh);
	if (P.window_radius == 2) {
		hipLaunchKernelGGL(mvs_reg_kernel<2>, dim3((unsigned)((n + 127)/128)), dim3(128), 0, st,
		                   views, ref, nl, nneigh, P, y0, nrows, wbuf, wstride, peaks, cnt);
		return;
	}
	hipLaunchKernelGGL(mvs_generic_kernel, dim3((unsigned)((n + 127)/128)), dim3(128), 0, st,
	                   views, ref, nl, nneigh, P, y0, nrows, wbuf, wstride, peaks, cnt);
}

// MultiViewStereo::crossCheck(view) (multiviewstereo.cpp:666-729)
__global__ void mvs_cross_check_kernel(const ViewDev *__restrict__ views, const int32_t *__restrict__ slots,
                                       int nviews, int view_index, srh_params P)
{
	const ViewDev &A = views[slots[view_index]];
	const int W = A.w, H = A.h;
	const size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= (size_t)W*H) return;
	const int x = (int)(i % W), y = (int)(i / W);
	const double depth = A.depth[i];
	if (!isfinite_d(depth)) return;
	const double s = P.image_scale;
	const Ray ray = cam_unproject(A.cam, (x + 0.5) / s, (y + 0.5) / s);
	Vec3 p1 = load3(A.cam.C);
	if (!point_from_depth(ray, load3(A.cam.pdir), depth, p1)) return;   // e.g. depth -1: left unchanged
	bool found = false;
	for (int v2 = 0; v2 < nviews && !found; ++v2) {
		if (v2 == view_index) continue;
		const ViewDev &B = views[slots[v2]];
		Vec3 q = p1;
		if (!cam_project(B.cam, q)) continue;
		const double x2 = q.x*s, y2 = q.y*s;
		if (!(x2 >= 0 && y2 >= 0 && x2 < B.w && y2 < B.h)) continue;
		const double odepth = B.depth[(size_t)((int)y2)*B.w + (int)x2];
		if (!isfinite_d(odepth)) continue;
		const Ray ray2 = cam_unproject(B.cam, (x2 + 0.5) / s, (y2 + 0.5) / s);
		Vec3 p2 = load3(B.cam.C);
		if (!point_from_depth(ray2, load3(B.cam.pdir), odepth, p2)) continue;
		const double nrm = norm(p1 - p2);
		if (isfinite_d(nrm) && nrm < P.cross_check_threshold) found = true;
	}
	if (!found) A.depth[i] = __builtin_nan("");
}

void launch_mvs_cross_check(hipStream_t st, const ViewDev *views, const int32_t *slots_dev, int nviews,
                            int view_index, int w, int h, const srh_params &P)
{
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(mvs_cross_check_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st,
	                   views, slots_dev, nviews, view_index, P);
}

} // namespace srh
