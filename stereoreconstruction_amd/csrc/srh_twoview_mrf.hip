// srh_twoview_mrf.hip -- the MRF stage of TwoViewStereo (twoviewstereo.cpp:240-258, 308-329, 335-403, 504-570; SURVEY
// 8(f) rank 2, second half): the per-label cost volume and sequential TRW-S over the 4-connected W x H grid with one
// label per depth level and the truncated-linear smoothness term lambda * min(|l1 - l2|, smooth_max).
//
// PARITY UNPINNED: the reference's branch is compile-time dead (#undef USE_MRF, :35), no longer compiles against its own
// cost_ncc signature and hands the energy to alpha-expansion from a library that is not in its tree.  FROM THE
// REFERENCE'S LINES: the labels and depthFromLabel, the label's pixel (pointFromDepth, project, times image_scale,
// truncated), the data cost (the live path's pair cost, WINDOW_SIZE*BAD_RET where a projection fails or the mask is not
// WHITE), the energy on the unmasked 4-connected grid, the start (messages zero, labels zero), the stopping loop and
// label -> depth.  OURS: the optimiser -- the TRW-S engine of sro_mvs_mrf (oracle/sr_oracle.c) with L = D labels --
// checked bit for bit against tests/twoview_mrf_restatement.cpp.  DESIGN.md 4d.
//
// The pass kernel keeps the structure of srh_mrf.hip: anti-diagonal order, one workgroup per band of 16 image rows taken
// by ticket (a band only ever waits for a band that started before it), the message to the right kept in registers, the
// message downward handed through LDS, a band's last row handed to the next band as self-validating {tag, half}
// granules, every spin bounded with a give-up status.  New is the label dimension: ONE WAVE PER IMAGE ROW of the band,
// the labels across its 64 lanes, NL = ceil(L/64) <= 4 consecutive labels per lane (label = lane*NL + j).  The
// truncated-linear message needs neither an O(L^2) loop nor a scan:
//     M[kd] = min( min_{|d| < smooth_max} (buf[kd + d] + lambda*|d|),  min_ks buf[ks] + lambda*smooth_max )
// -- the neighbours at distance <= 3 are in the lane or come from the two adjacent lanes (six shuffles per message,
// whatever NL), the second term is one wave-wide minimum.  These are the bits of the direct form: rounding is monotone,
// so min(a + c, b + c) and min(a, b) + c are the same number, and (lambda >= 0) a term with |d| < smooth_max that also
// enters the global minimum cannot lower it below its own windowed term.
// The computing waves store their own results (16 rows are 1024 threads: there is no room for the storing wave of
// srh_mrf.hip); every lane issues the same number of stores on every step (one without a destination goes to a trash row),
// so that the wait for the inputs fetched a step ahead is a fixed count and does not drain the stores behind them.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_window.hpp"
#include "srh_labels.hpp"

namespace srh {

namespace {

constexpr int TM_ROWS = 16;             // rows per band = waves per workgroup
constexpr int TM_THREADS = TM_ROWS*64;
constexpr int TM_LAG = 12;              // columns a band drops behind the one above once it had to wait for it
constexpr unsigned TM_SPIN_LIMIT = 1u << 21;

// sync block (4 unsigned words, zeroed before every pass): [0] ticket
// status block (zeroed once per run): [0] abort, [1] first band that gave up + 1, [2] pass it gave up in + 1
constexpr int SY_TICKET = 0;
constexpr int ST_ABORT = 0, ST_WHO = 1, ST_PASS = 2;

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the per-step barrier orders LDS only (srh_mrf.hip: the device-memory results go to other workgroups as granules or to
// the next launch)
__device__ __forceinline__ void tm_step_barrier() {
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// a double as two granules {tag, low half}, {tag, high half}: each one aligned 8-byte store (srh_mrf.hip)
__device__ __forceinline__ void put_granules(u64 *g, unsigned tag, double v) {
	const u64 bits = (u64)__double_as_longlong(v), t = (u64)tag << 32;
	__hip_atomic_store(g, t | (bits & 0xffffffffull), RLX_AGENT);
	__hip_atomic_store(g + 1, t | (bits >> 32), RLX_AGENT);
}
__device__ __forceinline__ u64 get_granule(const u64 *g) { return __hip_atomic_load(g, RLX_AGENT); }
__device__ __forceinline__ bool granules_ok(u64 g0, u64 g1, unsigned tag) { return (unsigned)(g0 >> 32) == tag && (unsigned)(g1 >> 32) == tag; }
__device__ __forceinline__ double granules_value(u64 g0, u64 g1) { return __longlong_as_double((long long)((g0 & 0xffffffffull) | (g1 << 32))); }

// smoothness cost between labels a and k: lambda * min(|a - k|, smooth_max) -- one product
__device__ __forceinline__ double tm_V(int a, int k, double lambda, double smax) {
	const double d = (double)(a > k ? a - k : k - a);
	return lambda*(d < smax ? d : smax);
}

template <int NL> struct Step {
	double D[NL], oH[NL], oV[NL];
	u64 g0[NL], g1[NL];                 // first row of a band: what the band above handed down (granules)
};

} // namespace

struct TvMrfPassArgs {
	int W, H, L, nwin;
	double lambda, smax, cmax, c[4];
	const double *D;                    // [n][L] data costs
	double *Mh, *Mv;                    // [n][L] message stored on the edge (n, n+1) / (n, n+W)
	int32_t *ans;                       // [n]
	double *trash;                      // [2][band][row][NL*64]: where a store without a destination goes (see the step's stores)
	unsigned long long *hand;           // [band][logical column][NL*64 label slots][2] granules out of each band's last row
	unsigned epoch;                     // tag of this pass: unique within a run, never 0
	unsigned *sync, *status;
};

// MODE 0: forward sweep, 1: backward sweep (logical coordinates mirrored), 2: labels read off (forward order)
// VEC: L is a multiple of NL and NL is even -- a lane moves its labels 16 bytes at a time
template <int MODE, int NL, bool VEC>
__global__ __launch_bounds__(TM_THREADS, 1) void twoview_mrf_pass_kernel(const TvMrfPassArgs a)
{
	constexpr int LP = NL*64;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	double *down = reinterpret_cast<double *>(smem);                                     // [2][row][LP]: message to the row below
	int *labs = reinterpret_cast<int *>(smem + (size_t)2*TM_ROWS*LP*sizeof(double));    // [2][row]: chosen label
	int *s_ctl = labs + 2*TM_ROWS;                                                       // [0] band, [1 + (step & 1)] a wait gave up

	const int tid = threadIdx.x, r = tid >> 6, lane = tid & 63;
	const int W = a.W, H = a.H, L = a.L;
	if (tid == 0) { s_ctl[0] = (int)atomicAdd(&a.sync[SY_TICKET], 1u); s_ctl[1] = 0; s_ctl[2] = 0; }
	__syncthreads();
	const int b = s_ctl[0];
	const int v = b*TM_ROWS + r;                                     // logical row
	const bool rowok = v < H;
	const int y = MODE == 1 ? H - 1 - v : v;
	const bool hasV = v < H - 1;                                     // an edge to the next logical row
	const int rlast = min(TM_ROWS, H - b*TM_ROWS) - 1;               // the band's last row
	const int nsteps = W + TM_ROWS - 1;
	const unsigned epoch = a.epoch;
	const bool takes = r == 0 && b > 0;                              // this wave's row is fed by the band above
	const double inf = __builtin_inf();
	const double lambda = a.lambda, smax = a.smax, cmax = a.cmax;
	const double cc[4] = { a.c[0], a.c[1], a.c[2], a.c[3] };
	const int nwin = a.nwin;
	bool lv[NL];
#pragma unroll
	for (int j = 0; j < NL; ++j) lv[j] = lane*NL + j < L;

	// physical pixel index of logical column u in this wave's row
	auto pix = [&](int u) -> long { return (long)y*W + (MODE == 1 ? W - 1 - u : u); };
	// granules the band above wrote for logical column u (label slot k; solve pass: slot 0, the one value of the pixel)
	auto hand_at = [&](int bb, int u, int k) -> u64 * { return a.hand + (((size_t)bb*W + u)*LP + k)*2; };

	auto fetch_granules = [&](int u, Step<NL> &B) -> bool {
		bool good = true;
		if (MODE == 2) {
			const u64 *g = hand_at(b - 1, u, 0);
			B.g0[0] = get_granule(g); B.g1[0] = get_granule(g + 1);
			good = granules_ok(B.g0[0], B.g1[0], epoch);
		} else {
#pragma unroll
			for (int j = 0; j < NL; ++j)
				if (lv[j]) {
					const u64 *g = hand_at(b - 1, u, lane*NL + j);
					B.g0[j] = get_granule(g); B.g1[j] = get_granule(g + 1);
					good = good && granules_ok(B.g0[j], B.g1[j], epoch);
				}
		}
		return good;
	};

	auto load_step = [&](int s, Step<NL> &B) {
		const int u = s - r;
		const bool ok = rowok && u >= 0 && u < W;
		const long n = pix(u);
		// the stored message on the edge towards the next logical column / row (written by the other sweep)
		const long eh = MODE == 1 ? n - 1 : n, ev = MODE == 1 ? n - W : n;
		if (VEC) {
			const bool okl = ok && lv[0];
			load_pieces<NL>(a.D + (n*L + lane*NL), okl, B.D);
			load_pieces<NL>(a.Mh + (eh*L + lane*NL), okl && u < W - 1, B.oH);
			load_pieces<NL>(a.Mv + (ev*L + lane*NL), okl && hasV, B.oV);
		}
#pragma unroll
		for (int j = 0; j < NL; ++j) {
			const int k = lane*NL + j;
			const bool okl = ok && lv[j];
			if (!VEC) {
				B.D[j] = okl ? a.D[n*L + k] : 0.0;
				B.oH[j] = (okl && u < W - 1) ? a.Mh[eh*L + k] : 0.0;
				B.oV[j] = (okl && hasV) ? a.Mv[ev*L + k] : 0.0;
			}
			B.g0[j] = 0; B.g1[j] = 0;
		}
		if (takes && ok) (void)fetch_granules(u, B);
	};

	// wave 0, before a step is computed: are the granules of its column this pass's?  If not: wait until the band above is
	// TM_LAG columns further and fetch them again (until they are: stores of one wave need not land in order).
	auto settle = [&](int s, Step<NL> &B) {
		const int u = s;                                              // (r == 0)
		if (u >= W) return;
		bool good = true;
		if (MODE == 2) good = granules_ok(B.g0[0], B.g1[0], epoch);
		else {
#pragma unroll
			for (int j = 0; j < NL; ++j) if (lv[j]) good = good && granules_ok(B.g0[j], B.g1[j], epoch);
		}
		if (__all(good)) return;
		const int ufar = min(u + TM_LAG, W - 1);
		unsigned spins = 0;
		int ok = 1;
		for (;;) {
			bool far = true;
			if (MODE == 2) { const u64 *g = hand_at(b - 1, ufar, 0); far = granules_ok(get_granule(g), get_granule(g + 1), epoch); }
			else {
#pragma unroll
				for (int j = 0; j < NL; ++j)
					if (lv[j]) { const u64 *g = hand_at(b - 1, ufar, lane*NL + j); far = far && granules_ok(get_granule(g), get_granule(g + 1), epoch); }
			}
			good = fetch_granules(u, B);
			if (__all(far && good)) break;
			if (++spins > TM_SPIN_LIMIT || __hip_atomic_load(&a.status[ST_ABORT], RLX_AGENT)) { ok = 0; break; }   // uniform
			__builtin_amdgcn_s_sleep(4);
		}
		if (!ok && lane == 0) {
			__hip_atomic_store(&a.status[ST_ABORT], 1u, RLX_AGENT);
			if (atomicCAS(&a.status[ST_WHO], 0u, (unsigned)b + 1u) == 0u) a.status[ST_PASS] = MODE + 1;
			s_ctl[1 + (s & 1)] = 1;
		}
	};

	// this wave's trash rows as offsets from the planes the stores go through (one allocation: the differences are plain numbers)
	const long trashH = (a.trash + ((size_t)b*TM_ROWS + r)*LP) - a.Mh;
	const long trashV = (a.trash + ((size_t)(gridDim.x + b)*TM_ROWS + r)*LP) - a.Mv;
	const long trashA = reinterpret_cast<int32_t *>(a.trash + ((size_t)b*TM_ROWS + r)*LP) - a.ans;
	Step<NL> cur, nxt;
	load_step(0, nxt);
	// (as many stores behind the first loads as every later step puts behind its own: the wait at the head of the step
	// loop is one count for both ways into it)
	if (MODE == 2) { long oA = trashA + lane; asm volatile("" : "+v"(oA)); a.ans[oA] = 0; }
	else {
#pragma unroll
		for (int j = 0; j < NL; j += VEC ? 2 : 1) {
			long oH = trashH + lane*NL + j, oV = trashV + lane*NL + j;
			asm volatile("" : "+v"(oH), "+v"(oV));
			if (VEC) { *reinterpret_cast<double2 *>(a.Mh + oH) = make_double2(0.0, 0.0); *reinterpret_cast<double2 *>(a.Mv + oV) = make_double2(0.0, 0.0); }
			else { a.Mh[oH] = 0.0; a.Mv[oV] = 0.0; }
		}
	}
	double carry[NL];                                                // message handed along the row
#pragma unroll
	for (int j = 0; j < NL; ++j) carry[j] = 0.0;
	int carry_lab = 0;                                               // solve pass: the left neighbour's label

	for (int s = 0; s < nsteps; ++s) {
		cur = nxt;
		if (takes) settle(s, cur);
		if (s + 1 < nsteps) load_step(s + 1, nxt);
		const int u = s - r;
		const bool ok = rowok && u >= 0 && u < W;
		const long n = pix(u);
		const int par = s & 1;
		const double *top = down + ((size_t)((s + 1) & 1)*TM_ROWS + (r > 0 ? r - 1 : 0))*LP;
		double *mine = down + ((size_t)par*TM_ROWS + r)*LP;

		if (MODE == 2) {
			// Di = D + V(left's label, .) + V(upper label, .) + message from the right + message from below
			int up_lab = 0;
			if (r > 0) up_lab = labs[((s + 1) & 1)*TM_ROWS + r - 1];
			else if (b > 0) up_lab = (int)granules_value(cur.g0[0], cur.g1[0]);
			double best = inf;
			int lab = 0x7fffffff;
#pragma unroll
			for (int j = 0; j < NL; ++j) {
				const int k = lane*NL + j;
				double Di = cur.D[j];
				if (u > 0) Di += tm_V(carry_lab, k, lambda, smax);
				if (v > 0) Di += tm_V(up_lab, k, lambda, smax);
				Di += cur.oH[j];
				Di += cur.oV[j];
				if (lv[j] && (lab == 0x7fffffff || best > Di)) { best = Di; lab = k; }
			}
			wave_argmin(best, lab);
			carry_lab = lab;
			if (lane == 0) labs[par*TM_ROWS + r] = lab;
			if (lane == 0 && ok && r == rlast && hasV) put_granules(hand_at(b, u, 0), epoch, (double)lab);
			long oA = (lane == 0 && ok) ? n : trashA + lane;            // (one store on every path, as below)
			asm volatile("" : "+v"(oA));
			a.ans[oA] = lab;
		} else {
			double Di[NL], bufH[NL], bufV[NL], mH[NL], mV[NL];
#pragma unroll
			for (int j = 0; j < NL; ++j) {
				const double fromL = u > 0 ? carry[j] : 0.0;
				const double fromT = r == 0 ? (b > 0 ? granules_value(cur.g0[j], cur.g1[j]) : 0.0) : top[lane*NL + j];
				double d = cur.D[j];
				if (MODE == 0) { d += fromL; d += fromT; d += cur.oH[j]; d += cur.oV[j]; }   // left, up, right, down
				else           { d += cur.oH[j]; d += cur.oV[j]; d += fromL; d += fromT; }
				Di[j] = d;
			}
			if (MODE == 1) {
				double vmin = inf;
#pragma unroll
				for (int j = 0; j < NL; ++j) if (lv[j]) vmin = vmin > Di[j] ? Di[j] : vmin;
				vmin = wave_min(vmin);
#pragma unroll
				for (int j = 0; j < NL; ++j) Di[j] -= vmin;
			}
#pragma unroll
			for (int j = 0; j < NL; ++j) {
				bufH[j] = lv[j] ? 0.5*Di[j] - cur.oH[j] : inf;
				bufV[j] = lv[j] ? 0.5*Di[j] - cur.oV[j] : inf;
			}
			trunc_message<NL>(bufH, lane, nwin, cc, cmax, mH);
			trunc_message<NL>(bufV, lane, nwin, cc, cmax, mV);
			double dH = inf, dV = inf;
#pragma unroll
			for (int j = 0; j < NL; ++j) if (lv[j]) { dH = dH > mH[j] ? mH[j] : dH; dV = dV > mV[j] ? mV[j] : dV; }
			dH = wave_min(dH); dV = wave_min(dV);
			// Every lane stores both messages of every label slot on every step, a store without a destination (outside the
			// image, a label that does not exist, no such edge) into the band's trash rows: the number of stores behind the
			// prefetching loads is then the same on every path, and the wait for the loads does not have to drain the stores.
			const long eh = MODE == 1 ? n - 1 : n, ev = MODE == 1 ? n - W : n;
#pragma unroll
			for (int j = 0; j < NL; ++j) {
				const int k = lane*NL + j;
				mH[j] -= dH; mV[j] -= dV;
				carry[j] = mH[j];
				mine[k] = mV[j];
				const bool toH = ok && lv[j] && u < W - 1, toV = ok && lv[j] && hasV;
				if (toV && r == rlast) put_granules(hand_at(b, u, k), epoch, mV[j]);
				if (!VEC) {
					long oH = toH ? eh*L + k : trashH + k, oV = toV ? ev*L + k : trashV + k;
					asm volatile("" : "+v"(oH), "+v"(oV));               // (one store each, not a store per branch of the selects)
					a.Mh[oH] = mH[j];
					a.Mv[oV] = mV[j];
				}
			}
			if (VEC) {
				const bool toH = ok && lv[0] && u < W - 1, toV = ok && lv[0] && hasV;
				long oH = toH ? eh*L + lane*NL : trashH + lane*NL, oV = toV ? ev*L + lane*NL : trashV + lane*NL;
				asm volatile("" : "+v"(oH), "+v"(oV));
				store_pieces<NL>(a.Mh + oH, mH);
				store_pieces<NL>(a.Mv + oV, mV);
			}
		}
		tm_step_barrier();
		if (s_ctl[1 + (s & 1)]) break;                               // a wait gave up: leave (results are reported invalid)
	}
}

// totalEnergy() of the current labels: one term set per pixel (its data cost, its edges to the left and up), summed per block
__global__ __launch_bounds__(256) void twoview_mrf_energy_kernel(int W, int H, int L, double lambda, double smax, const double *__restrict__ D,
                                                                 const int32_t *__restrict__ ans, double *__restrict__ partial)
{
	__shared__ double red[256];
	const long n = (long)blockIdx.x*256 + threadIdx.x;
	double e = 0.0;
	if (n < (long)W*H) {
		const int x = (int)(n % W), y = (int)(n / W);
		const int k = ans[n];
		e = D[n*L + k];
		if (x > 0) e += tm_V(k, ans[n - 1], lambda, smax);
		if (y > 0) e += tm_V(k, ans[n - W], lambda, smax);
	}
	red[threadIdx.x] = e;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// fixed-shape sum of the per-block partials (one block): same bits on every run
__global__ __launch_bounds__(1024) void twoview_mrf_energy_sum_kernel(int nparts, const double *__restrict__ partial, double *__restrict__ out)
{
	__shared__ double red[1024];
	double e = 0.0;
	for (int i = threadIdx.x; i < nparts; i += 1024) e += partial[i];
	red[threadIdx.x] = e;
	__syncthreads();
	for (int s = 512; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0) *out = red[0];
}

// label -> depth: depthFromLabel(label) where the mask is WHITE (twoviewstereo.cpp:324), NaN elsewhere
__global__ void twoview_mrf_depth_kernel(const ViewDev *__restrict__ views, int slot, srh_params P, const int32_t *__restrict__ ans)
{
	const ViewDev &V = views[slot];
	const long n = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (n >= (long)V.w*V.h) return;
	V.depth[n] = V.mask[n] == 1 ? depth_from_label(P, false, ans[n]) : __builtin_nan("");
}

// The label cost volume of rows [y0, y0 + nrows).  A workgroup takes 64 consecutive reference pixels: its first wave builds
// their support windows in LDS, one lane per pixel (tap-major with a stride of 64: support_window, the bits of the weights
// kernels); then each of its LC_PARTS waves takes a contiguous share of the labels of the same 64 pixels, a lane per pixel:
// the walk's own projection (walk_curve: pointFromDepth, project, times image_scale, truncated by trunc_sat) and the
// reference-form pair cost of srh_walk.hpp -- the very functions pair_costs_kernel evaluates.  Consecutive labels of a
// share that fall on one pixel share the cost.
#define LC_LANES 64
#define LC_PARTS 4
#define LC_TAPS 121
__global__ __launch_bounds__(LC_LANES*LC_PARTS)
void twoview_label_costs_kernel(const ViewDev *__restrict__ views, int ref, int oth, srh_params P, int kind, int y0, int nrows,
                                double fill, double *__restrict__ cost, int32_t *__restrict__ pixel)
{
	__shared__ double wl[LC_TAPS*LC_LANES];
	const int lane = threadIdx.x & (LC_LANES - 1), part = threadIdx.x / LC_LANES;
	const ViewDev &L = views[ref];
	const ViewDev &Rv = views[oth];
	const int W = L.w, D = P.num_depth_levels;
	const long q = (long)blockIdx.x*LC_LANES + lane;
	const bool inside = q < (long)nrows*W;
	const int x = inside ? (int)(q % W) : 0, y = inside ? y0 + (int)(q / W) : y0;
	const bool white = inside && L.mask[(size_t)y*W + x] == 1;
	const int WS = 2*P.window_radius + 1;
	double *wb = wl + lane;
	if (part == 0 && white) support_window(L, P, x, y, [&](int r, int c) -> double & { return wb[(r*WS + c)*LC_LANES]; });
	__syncthreads();
	if (!inside) return;
	const int d0 = (int)((long)D*part/LC_PARTS), d1 = (int)((long)D*(part + 1)/LC_PARTS);
	double *out = cost + q*D;
	int32_t *pout = pixel ? pixel + q*D*2 : nullptr;
	if (!white) {                                                     // never costed (:270-271): std::fill's value stays
		for (int d = d0; d < d1; ++d) { out[d] = fill; if (pout) { pout[2*d] = SRH_LABEL_PIXEL_NONE; pout[2*d + 1] = SRH_LABEL_PIXEL_NONE; } }
		return;
	}
	const Ray ray = cam_unproject(L.cam, (x + 0.5) / P.image_scale, (y + 0.5) / P.image_scale);
	const Vec3 camC = load3(L.cam.C);
	const Vec3 normal = load3(L.cam.pdir);
	const Vec3 oth_bn = normalized(load3(Rv.cam.plane_normal));
	bool have = false;
	int lx = 0, ly = 0;
	double lcost = 0.0;
	for (int d = d0; d < d1; ++d) {
		Vec3 point = camC;
		const double depth = depth_from_label(P, false, d);
		bool okp = point_from_depth(ray, normal, depth, point);
		if (okp) okp = cam_project(Rv.cam, point, &oth_bn);
		if (!okp) {
			out[d] = fill;
			if (pout) { pout[2*d] = SRH_LABEL_PIXEL_NONE; pout[2*d + 1] = SRH_LABEL_PIXEL_NONE; }
			continue;
		}
		const int x2 = trunc_sat(point.x*P.image_scale), y2 = trunc_sat(point.y*P.image_scale);
		if (!(have && x2 == lx && y2 == ly)) {
			lcost = tv_cost_of(kind, L, Rv, wb, LC_LANES, P, x, y, x2, y2);
			lx = x2; ly = y2; have = true;
		}
		out[d] = lcost;
		if (pout) { pout[2*d] = x2; pout[2*d + 1] = y2; }
	}
}

static TvMrfPassArgs carve(double *buf, int w, int h, int L, TvMrfLayout &lay)
{
	const size_t n = (size_t)w*h, nr = (n + 1) & ~(size_t)1;           // every block starts 16-byte aligned
	const int NL = (L + 63)/64;
	const size_t vol = (n*(size_t)L + 1) & ~(size_t)1;
	lay.Mh = buf; lay.Mv = buf + vol;
	lay.nbands = (h + TM_ROWS - 1)/TM_ROWS;
	lay.hand = reinterpret_cast<unsigned long long *>(buf + 2*vol);
	lay.hand_words = (size_t)lay.nbands*w*(size_t)(NL*64)*2;
	lay.trash = buf + 2*vol + lay.hand_words;
	lay.partial = lay.trash + (size_t)2*lay.nbands*TM_ROWS*(size_t)(NL*64);
	lay.nparts = (int)((n + 255)/256);
	lay.energy = lay.partial + ((lay.nparts + 1) & ~1);                // [0] energy, [1] unused
	lay.status = reinterpret_cast<unsigned *>(lay.energy + 2);         // 4 words
	lay.ans = reinterpret_cast<int32_t *>(lay.energy + 4);
	lay.sync = reinterpret_cast<unsigned *>(lay.ans + nr);
	lay.sync_words = 4;
	lay.total_doubles = (size_t)(reinterpret_cast<double *>(lay.sync) - buf) + lay.sync_words/2;
	TvMrfPassArgs a;
	a.W = w; a.H = h; a.L = L;
	a.Mh = lay.Mh; a.Mv = lay.Mv; a.ans = lay.ans; a.trash = lay.trash; a.hand = lay.hand; a.epoch = 0;
	a.sync = lay.sync; a.status = lay.status;
	return a;
}

void launch_twoview_mrf_layout(double *buf, int w, int h, int L, TvMrfLayout &lay) { carve(buf, w, h, L, lay); }

size_t twoview_mrf_scratch_doubles(int w, int h, int L)
{
	TvMrfLayout lay;
	carve(nullptr, w, h, L, lay);
	return lay.total_doubles;
}

// initialize(): messages 0; clearAnswer(): label 0; the status words; no granule tag is 0
hipError_t launch_twoview_mrf_setup(hipStream_t st, double *buf, int w, int h, int L, TvMrfLayout &lay)
{
	carve(buf, w, h, L, lay);
	const size_t n = (size_t)w*h;
	hipError_t e;
	if ((e = hipMemsetAsync(lay.Mh, 0, (size_t)(reinterpret_cast<char *>(lay.hand) - reinterpret_cast<char *>(lay.Mh)), st)) != hipSuccess) return e;
	if ((e = hipMemsetAsync(lay.ans, 0, n*sizeof(int32_t), st)) != hipSuccess) return e;
	if ((e = hipMemsetAsync(lay.energy, 0, 4*sizeof(double), st)) != hipSuccess) return e;
	return hipMemsetAsync(lay.hand, 0, lay.hand_words*sizeof(unsigned long long), st);
}

template <int MODE, int NL, bool VEC> static hipError_t launch_pass_nl(hipStream_t st, const TvMrfPassArgs &a, const TvMrfLayout &lay)
{
	const size_t lds = (size_t)2*TM_ROWS*NL*64*sizeof(double) + (2*TM_ROWS + 4)*sizeof(int);
	hipError_t e;
	if ((e = hipMemsetAsync(lay.sync, 0, lay.sync_words*sizeof(unsigned), st)) != hipSuccess) return e;
	if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(&twoview_mrf_pass_kernel<MODE, NL, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize,
	                             (int)lds)) != hipSuccess) return e;
	hipLaunchKernelGGL((twoview_mrf_pass_kernel<MODE, NL, VEC>), dim3((unsigned)lay.nbands), dim3(TM_THREADS), lds, st, a);
	return hipGetLastError();
}
template <int MODE> static hipError_t launch_pass(hipStream_t st, const TvMrfPassArgs &a, const TvMrfLayout &lay)
{
	// the 16-byte form needs the volume on a 16-byte boundary as well (the planes of the scratch buffer are)
	const bool vec = (reinterpret_cast<uintptr_t>(a.D) & 15) == 0;
	switch ((a.L + 63)/64) {
	case 1: return launch_pass_nl<MODE, 1, false>(st, a, lay);
	case 2: return vec && a.L % 2 == 0 ? launch_pass_nl<MODE, 2, true>(st, a, lay) : launch_pass_nl<MODE, 2, false>(st, a, lay);
	case 3: return launch_pass_nl<MODE, 3, false>(st, a, lay);
	default: return vec && a.L % 4 == 0 ? launch_pass_nl<MODE, 4, true>(st, a, lay) : launch_pass_nl<MODE, 4, false>(st, a, lay);
	}
}

// one sweep: forward, backward, labels read off.  `sweep` (0, 1, ...) numbers the calls of one run: every pass gets a
// granule tag of its own
hipError_t launch_twoview_mrf_sweep(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax, int sweep)
{
	TvMrfLayout lay;
	TvMrfPassArgs a = carve(buf, w, h, L, lay);
	a.D = costs;
	a.lambda = lambda; a.smax = smax; a.cmax = lambda*smax;
	for (int d = 0; d < 4; ++d) a.c[d] = lambda*(double)d;
	a.nwin = 0;
	while (a.nwin < 3 && (double)(a.nwin + 1) < smax) ++a.nwin;        // the largest d < smooth_max
	hipError_t e;
	a.epoch = 1u + 3u*(unsigned)sweep;
	if ((e = launch_pass<0>(st, a, lay)) != hipSuccess) return e;
	a.epoch += 1;
	if ((e = launch_pass<1>(st, a, lay)) != hipSuccess) return e;
	a.epoch += 1;
	return launch_pass<2>(st, a, lay);
}

// totalEnergy() into lay.energy[0]; the status words follow it (lay.status)
hipError_t launch_twoview_mrf_energy(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax)
{
	TvMrfLayout lay;
	carve(buf, w, h, L, lay);
	hipLaunchKernelGGL(twoview_mrf_energy_kernel, dim3((unsigned)lay.nparts), dim3(256), 0, st, w, h, L, lambda, smax, costs, lay.ans, lay.partial);
	hipLaunchKernelGGL(twoview_mrf_energy_sum_kernel, dim3(1), dim3(1024), 0, st, lay.nparts, lay.partial, lay.energy);
	return hipGetLastError();
}

// the same energy of any labelling `ans` of the grid (srh_twoview_sgm.hip): partial holds nparts = ceil(w*h/256) doubles
hipError_t launch_twoview_labels_energy(hipStream_t st, const double *costs, const int32_t *ans, double *partial, int nparts, double *energy,
                                        int w, int h, int L, double lambda, double smax)
{
	hipLaunchKernelGGL(twoview_mrf_energy_kernel, dim3((unsigned)nparts), dim3(256), 0, st, w, h, L, lambda, smax, costs, ans, partial);
	hipLaunchKernelGGL(twoview_mrf_energy_sum_kernel, dim3(1), dim3(1024), 0, st, nparts, partial, energy);
	return hipGetLastError();
}

hipError_t launch_twoview_mrf_depth(hipStream_t st, const ViewDev *views, int slot, const srh_params &P, double *buf, int w, int h, int L)
{
	TvMrfLayout lay;
	carve(buf, w, h, L, lay);
	const size_t n = (size_t)w*h;
	hipLaunchKernelGGL(twoview_mrf_depth_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st, views, slot, P, lay.ans);
	return hipGetLastError();
}

hipError_t launch_twoview_label_costs(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int kind,
                                      int y0, int nrows, double fill, double *cost, int32_t *pixel)
{
	const size_t n = (size_t)nrows*width;
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(twoview_label_costs_kernel, dim3((unsigned)((n + LC_LANES - 1)/LC_LANES)), dim3(LC_LANES*LC_PARTS), 0, st,
	                   views, ref, oth, P, kind, y0, nrows, fill, cost, pixel);
	return hipGetLastError();
}

} // namespace srh
