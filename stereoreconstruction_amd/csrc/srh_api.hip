// srh_api.hip -- the C-ABI of include/stereo_recon_hip.h: context, view upload,
// run entry points, measurement.  Host code only; every numeric result comes from
// the kernels in srh_kernels.hip / srh_mvs.hip / srh_dense.hip.  There is no CPU fallback: without
// a HIP device srh_create fails with SRH_E_NO_DEVICE.
#include "srh_internal.hpp"
#include "srh_subpixel.hpp"
#include "srh_mvs_subpixel.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"
#include "srh_speckle.hpp"
#include "srh_rectify.hpp"

#include <algorithm>
#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <limits>
#include <vector>

using namespace srh;

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return code;
}

#define HIP_TRY(expr)                                                                   \
	do {                                                                                \
		hipError_t e_ = (expr);                                                         \
		if (e_ != hipSuccess)                                                           \
			return fail(SRH_E_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
	} while (0)

// ------------------------------------------------------------------ device memory
// Band buffers grow on demand.  A request the device cannot serve is not the end of the call: g_oom tells the entry
// point (with_thinner_bands below) to release the band buffers, halve the band budget and run again.
// g_alloc_limit (option "debug_alloc_limit_mb") makes requests above a size fail the same way: the test of that path.
// (both are set from the context at the start of every retrying entry point -- with_thinner_bands -- so that a limit set
// through one thread applies to calls made on another)
static thread_local bool g_oom = false;
static thread_local size_t g_alloc_limit = 0;

// ---- the process's pool of device blocks -----------------------------------------------------------------------------
// A TwoViewStereo / MultiViewStereo object of the reference lives for one computation (twoviewstereo.cpp:150-227; the GUI
// makes a new one per run), so a drop-in creates and destroys contexts again and again in one process -- and a context's
// band buffers are gigabytes.  Handing them back to the driver at srh_destroy and asking for them again at the next
// object's first call is not free on this stack: measured (profiles/r06_first_call.txt, HIP API trace) ONE hipMalloc of 11 GB
// now and then takes 0.9 ... 1.5 s when tens of GB have just been freed by the same process (its siblings: 0.3 ms).  So band
// buffers and view planes (230 MB for a 1920 x 1080 view) released by srh_destroy, free_view or a growing buffer go to a
// process-wide pool, per device, under their real size, and the next context's requests are served from it (best fit, at
// most 1.5x the request); what is under the floor or does not fit the pool's cap is freed.  The pool is emptied before an
// allocation is declared out of memory, and counts as available memory for the band planner.
// Option "band_pool_mb" (any context; process-wide): the cap, default 65 536; 0 empties and disables the pool.
struct PoolBlock { void *p; size_t bytes; int device; };
static std::mutex g_pool_mu;
static std::vector<PoolBlock> g_pool;
static size_t g_pool_bytes = 0, g_pool_cap = (size_t)65536 << 20;
static const size_t POOL_MIN_BYTES = (size_t)4 << 20;                // smaller buffers are not worth a pool entry

static void pool_flush(int device) {                                 // (device < 0: every device)
	std::vector<PoolBlock> out;
	{
		std::lock_guard<std::mutex> g(g_pool_mu);
		for (size_t k = 0; k < g_pool.size();)
			if (device < 0 || g_pool[k].device == device) { out.push_back(g_pool[k]); g_pool_bytes -= g_pool[k].bytes; g_pool[k] = g_pool.back(); g_pool.pop_back(); }
			else ++k;
	}
	int cur = 0;
	const bool have = hipGetDevice(&cur) == hipSuccess;
	for (const PoolBlock &b : out) { (void)hipSetDevice(b.device); (void)hipFree(b.p); }
	if (have) (void)hipSetDevice(cur);
}
static size_t pool_bytes_on(int device) {
	std::lock_guard<std::mutex> g(g_pool_mu);
	size_t b = 0;
	for (const PoolBlock &k : g_pool) if (k.device == device) b += k.bytes;
	return b;
}
// a released block of `bytes` on the current device: into the pool, or back to the driver
static void pool_give(void *p, size_t bytes) {
	if (!p) return;
	int dev = 0;
	if (bytes >= POOL_MIN_BYTES && hipGetDevice(&dev) == hipSuccess) {
		std::lock_guard<std::mutex> g(g_pool_mu);
		if (g_pool_bytes + bytes <= g_pool_cap) { g_pool.push_back({p, bytes, dev}); g_pool_bytes += bytes; return; }
	}
	(void)hipFree(p);
}
// a block of at least `bytes` (at most 1.5x) from the pool, or null; *got = its size
static void *pool_take(size_t bytes, size_t *got) {
	int dev = 0;
	if (bytes < POOL_MIN_BYTES || hipGetDevice(&dev) != hipSuccess) return nullptr;
	std::lock_guard<std::mutex> g(g_pool_mu);
	size_t best = g_pool.size();
	for (size_t k = 0; k < g_pool.size(); ++k)
		if (g_pool[k].device == dev && g_pool[k].bytes >= bytes && g_pool[k].bytes <= bytes + bytes/2 &&
		    (best == g_pool.size() || g_pool[k].bytes < g_pool[best].bytes)) best = k;
	if (best == g_pool.size()) return nullptr;
	void *p = g_pool[best].p;
	*got = g_pool[best].bytes;
	g_pool_bytes -= g_pool[best].bytes;
	g_pool[best] = g_pool.back(); g_pool.pop_back();
	return p;
}

// Every device block of this file: from the pool, else from the driver -- and after an out-of-memory answer once more,
// with this device's pool given back first (the pool's blocks are memory too).  *got = the block's real size.
static hipError_t dev_alloc(void **p, size_t bytes, size_t *got) {
	if ((*p = pool_take(bytes, got))) return hipSuccess;
	hipError_t e = hipMalloc(p, bytes);
	if (e == hipErrorOutOfMemory) {
		(void)hipGetLastError();
		int dev = 0;
		if (hipGetDevice(&dev) == hipSuccess && pool_bytes_on(dev)) { pool_flush(dev); e = hipMalloc(p, bytes); }
	}
	if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return e; }
	*got = bytes;
	return hipSuccess;
}

// A device buffer: the block, its real size in bytes and the elements of T it holds.  Not copyable; a move leaves the source
// empty and goes into an empty buffer only, so no assignment drops a block.  Nothing frees it implicitly: release() (to
// the pool, whose floor and cap decide what waits there) and free() (to the driver) show where device memory leaves, and
// the device waits they need stay at their call sites.
template <class T>
struct DevBuf {
	T *p = nullptr;
	size_t n = 0, block = 0;
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
	DevBuf &operator=(DevBuf &&o) noexcept {
		assert(!p && "a held block is released, not overwritten");
		p = o.p; n = o.n; block = o.block;
		o.p = nullptr; o.n = o.block = 0;
		return *this;
	}
	operator T *() const { return p; }
	T *operator->() const { return p; }
	size_t bytes() const { return block; }
	// `count` elements into this empty buffer
	hipError_t alloc(size_t count) {
		void *q = nullptr;
		size_t got = 0;
		const hipError_t e = dev_alloc(&q, count*sizeof(T), &got);
		if (e == hipSuccess) { p = (T *)q; n = got/sizeof(T); block = got; }
		return e;
	}
	// a band buffer of at least `need` elements (kept when it holds them already)
	int ensure(size_t need) {
		if (n >= need) return SRH_OK;
		// (a buffer that is being outgrown: hipFree used to wait for the device before it let go of it; the pool must not hand it to
		// another context while a kernel queued earlier still reads it -- growth is rare, the wait is kept)
		if (p) { (void)hipDeviceSynchronize(); release(); }
		if (g_alloc_limit && need*sizeof(T) > g_alloc_limit) {
			g_oom = true;
			return fail(SRH_E_DEVICE, "band buffer of %zu bytes refused (debug_alloc_limit_mb)", need*sizeof(T));
		}
		const hipError_t e = alloc(need);
		if (e == hipErrorOutOfMemory) g_oom = true;
		if (e != hipSuccess) return fail(SRH_E_DEVICE, "hipMalloc of a %zu-byte band buffer: %s", need*sizeof(T), hipGetErrorString(e));
		return SRH_OK;
	}
	void release() { pool_give(p, block); p = nullptr; n = block = 0; }
	void free() { if (p) (void)hipFree(p); p = nullptr; n = block = 0; }
};

// The band buffers of one pass: scratch sized by the band height, which an out-of-memory retry gives back
// (release_band_buffers).  each() is the one list.
struct BandBuffers {
	DevBuf<double> wbuf;            // support windows of the band
	DevBuf<double> cost;            // cost rows of the band
	DevBuf<double> tnum;            // per-label table of the pinhole walk
	DevBuf<double> pconst;          // per-pixel constants of the dense kernel's fast form (4 doubles per pixel of a band)
	DevBuf<PixRange> prange;        // per-pixel candidate column range of a band (strip kernel, scan)
	DevBuf<uint32_t> filllist;      // [count | band pixels whose last columns the cost kernel leaves out] (pixel_range_kernel -> fill kernels)
	DevBuf<uint32_t> cflag;         // certified arithmetic: [count | band pixels whose decisions the bound does not cover]
	DevBuf<uint8_t> stpl;           // template scan: the pass's candidate template (twoview_template_kernel)
	DevBuf<uint32_t> tileflag;      //   and the tiles it leaves to twoview_scan_kernel: [count | tile indices]
	DevBuf<int32_t> lcount;         // candidate-list path: candidates per pixel
	DevBuf<uint32_t> lcand;         //   candidate pixels (cx | cy<<16)
	DevBuf<uint32_t> lrowinfo;      //   row runs of the lists (srh_rows.hip)
	DevBuf<int32_t> lmeta;
	DevBuf<uint32_t> mvs_wdesc;     // window descriptors of the MultiViewStereo walk kernel's waves
	DevBuf<int32_t> mvs_nwin;
	DevBuf<double> subpx_tdist;     // option "subpixel": per-label plane table of the neighbours kernel's walk
	template <class F> void each(F f) {
		f(wbuf); f(cost); f(tnum); f(pconst); f(prange); f(filllist); f(cflag); f(stpl); f(tileflag);
		f(lcount); f(lcand); f(lrowinfo); f(lmeta); f(mvs_wdesc); f(mvs_nwin); f(subpx_tdist);
	}
	size_t bytes() { size_t b = 0; each([&](auto &x) { b += x.bytes(); }); return b; }
	void release() { each([](auto &x) { x.release(); }); }
	void free() { each([](auto &x) { x.free(); }); }
};
// What a pass writes: its band buffers, its counters and the maxima of its list kernels (4 ints).  The context owns one
// set; the second TwoView pass (TvSlot) and the second MultiViewStereo estimate in flight (MvsSlot 1) own one each
// (srh_context::each_scratch is the one list).  Where a pass runs: a stream and the set it writes -- every runner, launcher
// and helper of a pass is handed its Lane (or the lane's stream) and reads neither from the context.
struct Scratch {
	BandBuffers band; DevBuf<Counters> cnt; DevBuf<int> span;
	void release() { band.release(); cnt.release(); span.release(); }
};
struct Lane { hipStream_t stream; Scratch *mem; };

// What a context keeps of one label-volume stage (an optimiser over a per-pixel label volume: TRW-S or semi-global
// aggregation, for MultiViewStereo's peak labels or TwoViewStereo's depth labels): the stage's scratch, for TwoViewStereo the
// label cost volume it computes itself, and what the last finished one-view run left in them, w x h pixels by l labels
// (K peaks or L depth levels), for the stage's *_dims and *_state.  w = 0: nothing to report.
struct LabelStage {
	const char *run_name, *last_name;       // "no finished <run_name> run", "the last <last_name> run was"
	char letter;                            // what the messages call the label count
	DevBuf<double> scratch, costs;
	int w = 0, h = 0, l = 0;
	bool own_costs = false;                 // the last run's data costs are in `costs`, not in a caller's volume
	void forget() { w = h = l = 0; }
	void forget_if(int vw, int vh) { if (w == vw && h == vh) forget(); }     // a view of that size got new pixels
	void finished(int w_, int h_, int l_) { w = w_; h = h_; l = l_; }
	void release() { scratch.release(); costs.release(); }
	int dims(int *w_out, int *h_out, int *l_out) const {                     // the last run's size, where asked for
		if (!w) return fail(SRH_E_INVALID, "no finished %s run on this context", run_name);
		if (w_out) *w_out = w;
		if (h_out) *h_out = h;
		if (l_out) *l_out = l;
		return SRH_OK;
	}
	int check_dims(int bw, int bh, int bl) const {                           // the caller's buffers are sized for it
		if (!w || (bw == w && bh == h && bl == l)) return dims(nullptr, nullptr, nullptr);
		return fail(SRH_E_INVALID, "buffers sized for %dx%d, %c = %d, the last %s run was %dx%d, %c = %d", bw, bh, letter, bl, last_name, w, h, letter, l);
	}
};

// ------------------------------------------------------------------ context
struct ViewHost {
	int w = 0, h = 0;
	bool present = false;
	DevBuf<uint32_t> rgba;
	DevBuf<uint8_t>  mask;
	DevBuf<double>   gray, gray_tv, depth;
	DevBuf<double>   edges;        // 4 planes of neighbour colour distances (geodesic windows)
	DevBuf<uint8_t>  full;         // 1 where the whole (2*full_r+1)^2 TwoView window is usable
	int              full_r = 0;
	// strip kernel (srh_strip.hip): NaN-bordered copy of gray_tv, zero-bordered "window fully usable" plane for radius fullp_r
	DevBuf<double>   tvp;   bool tvp_valid = false;
	DevBuf<double>   geo5;  bool geo5_valid = false;      // edge + tap planes with their borders written out (geodesic_dma_kernel)
	bool             geo5_denied = false;                 // released by an out-of-memory retry: this upload keeps the register-staged windows kernel
	DevBuf<uint8_t>  fullp; int fullp_r = 0;
	DevBuf<uint8_t>  fulls; int fulls_r = 0;            // cost_sad's "window fully usable" plane of radius fulls_r (srh_sad.hip): its own
	                                                      // validity (pixel() behind the mask), so never the NCC plane `full`
	// cost_sad on the dense plan (srh_sad_strip.hip): NaN-bordered copy of gray where the mask is WHITE, zero-bordered copy of `fulls`
	DevBuf<double>   grayp; bool grayp_valid = false;
	DevBuf<uint8_t>  fullsp; int fullsp_r = 0;
	// option "cost" = SRH_COST_CENSUS (srh_census.hip): the 9x7 census signatures of `gray`, made on first use after an upload
	DevBuf<uint64_t> census; bool census_valid = false;
	// the census cost on the dense plan (srh_census_strip.hip): `census` on the padded raster as the other side's taps (unusable
	// behind the mask) and as the reference side's (unusable where gray_tv is NaN)
	DevBuf<uint64_t> cenothp, cenrefp; bool cenp_valid = false;
	// how the candidate lists of this view against slot j are best evaluated, learnt from the last run:
	// 0 unknown, 1 row runs (srh_rows.hip), 2 list order (srh_list.hip: steep curves)
	uint8_t   list_mode[SRH_MAX_VIEWS] = {0};
	// MultiViewStereo list path: the masked-in pixels (y*w + x) row by row, even rows left to right, odd rows right to
	// left, so that consecutive entries are neighbours in the image also across a row change; act_row[y] = first entry of
	// row y (h + 1 values).  A wave of the walk / cost kernels takes 64 consecutive entries.
	DevBuf<uint32_t> act;
	std::vector<uint32_t> act_row, act_host;
	std::vector<uint8_t> hmask;    // host copy of the mask bytes (empty: no mask, every pixel counts): `act` is built from it
	bool act_valid = false;        //   when the MultiViewStereo list path first asks (ensure_act); TwoView callers never pay for it
	srh_camera cam;
	// MRF branch over several views (srh_mvs_initial_estimate_peaks / srh_mvs_mrf_estimate_views)
	// by-products of the last TwoView WTA pass with this view as the reference (option "wta_outputs"):
	// win_xy | runner_xy (2 int32 each per pixel) and min_cost | second_cost, allocated by the first pass that keeps them
	DevBuf<int32_t> wta_xy;
	DevBuf<double>  wta_cost;
	int wta_flags = 0, wta_oth = -1;            // what the planes hold (SRH_WTA_*; 0: nothing, or stale) and against which slot
	int wta_asked = 0;                          // of wta_flags, what option "wta_outputs" asked for: what the getters show (option "subpixel" keeps all)
	// option "subpixel" (DESIGN.md 4n): delta, (n-, n+) and the class of every pixel of that pass; subpx: the pass refined
	DevBuf<double>  subpx_delta;
	DevBuf<int32_t> subpx_neigh;
	DevBuf<uint8_t> subpx_cls;
	bool subpx = false;
	DevBuf<double> peaks; int peaks_k = 0;      // top-K peaks of the last initial estimate
	DevBuf<double> mrf;                         // this view's own TRW-S scratch
	DevBuf<double> sgm;                         // this view's own aggregation scratch (srh_mvs_sgm_estimate_views)
};

struct ProfEntry { double ms = 0; int64_t n = 0; };
struct PendingEvt { std::string name; hipEvent_t a, b; };

#ifndef SRH_MVS_SLOTS
#define SRH_MVS_SLOTS 2
#endif
// one MultiViewStereo estimate in flight (srh_mvs_initial_estimate, "two estimates in flight")
struct MvsSlot {
	hipStream_t stream = nullptr;
	hipEvent_t ev = nullptr, done = nullptr;
	int *h_maxc = nullptr;                              // pinned: longest list of the queued pass
	bool own_buffers = false;                           // slot 1: its own scratch; slot 0 runs on the context's
	Scratch mem;
	bool pending = false;                               // kernels queued, capacity check outstanding
	int view = -1, nneigh = 0, y0 = 0, y1 = 0, cmax = 0;
	int32_t neigh[SRH_MAX_NEIGH] = {0};
	srh_params p;
};

struct srh_context {
	int device = 0;
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;
	ViewHost views[SRH_MAX_VIEWS];
	DevBuf<ViewDev> d_views;
	DevBuf<int32_t> d_slots;
	int32_t slots_host[SRH_MAX_VIEWS] = {0}; int slots_n = 0;   // what d_slots holds (srh_mvs_cross_check: the same list for every view of a run)
	Scratch mem;                                        // the context's own scratch: with `stream`, the main lane
	hipStream_t mrf_stream[SRH_MAX_VIEWS] = { nullptr };            // one stream per view of srh_mvs_mrf_estimate_views / _sgm_
	hipEvent_t views_go = nullptr;                                  //   which start behind this event on the context's stream
	void *mrf_host = nullptr;                                       // pinned: per view {energy, pad, status[4]}
	DevBuf<double> mrf_peaks;                           // top-K peaks of srh_mvs_initial_estimate_mrf
	DevBuf<double> mvs_subpx;                           // srh_mvs_view_subpixel: the call's counters and planes (allocated by the first call)
	int mvs_subpx_search = 0;                           // option "mvs_subpixel_search": 1 = the winner search is exhaustive for every pixel
	double *mvsgm_host = nullptr;                       // pinned: one energy per view of the MultiView aggregation
	// the label-volume stages (LabelStage above): the scratch of each is carved by its kernel file's layout
	LabelStage mrf   { "single-view MRF", "MRF", 'K' };             // MultiViewStereo TRW-S (srh_mrf.hip)
	LabelStage mvsgm { "single-view SGM", "SGM", 'K' };             // MultiViewStereo semi-global aggregation (srh_mvs_sgm.hip)
	LabelStage tvmrf { "TwoView MRF", "TwoView MRF", 'L' };         // TwoViewStereo TRW-S (srh_twoview_mrf.hip)
	LabelStage tvsgm { "TwoView SGM", "TwoView SGM", 'L' };         // TwoViewStereo semi-global aggregation (srh_twoview_sgm.hip)
	LabelStage *const label_stages[4] = { &mrf, &mvsgm, &tvmrf, &tvsgm };
	int geodma = 1;                                     // option "geodma": 1 = the dense path's r = 5 geodesic windows by the persistent LDS-DMA kernel (default), 0 = geodesic_reg_kernel
	int tscan_bound = 1;                                // option "tscan_bound": 1 = the template scan settles a pixel by ONE bound for all its labels (default), 0 = label by label
	int tscan = 1;                                      // option "tscan": 1 = template scan on the dense path (default), 0 = every tile through twoview_scan_kernel
	int strip = 1;                                      // option "strip": 1 = persistent strip cost kernel (default), 0 = one workgroup per tile, 4 / 8 = force the 4- / 8-wave form
	int num_cus = 256;
	bool force_walk = false;                            // option "force_generic" = 2: never use the list path either
	int list_count_pass = 0;                            // option "list_count_pass": size a pair's first lists by a counting pass (round 5) instead of the host's guess
	int list_cmax_hint = 0;                             // longest candidate list seen so far (list-path capacity)
	int list_smax_hint = 0;                             // most cost slots a pixel needed so far (run-blocked lists)
	int mvs_cmax_hint = 0;                              // longest MultiViewStereo candidate list seen so far
	// side stream of the row-run list path: the support windows are computed while the list kernel's last waves drain
	hipStream_t side_stream = nullptr;
	hipEvent_t side_go = nullptr, side_done = nullptr;
	hipEvent_t side_tpl = nullptr;                      // dense plan: the scan template, made on the side stream behind the range kernel
	int mvs_async = 1;                                  // option "mvs_async": srh_mvs_initial_estimate queues a view on one of two side streams and returns (default); 0 = waits for each view
	MvsSlot mvs_slot[SRH_MVS_SLOTS];
	int mvs_turn = 0, mvs_last = -1;
	int mvs_staged = 1;                                 // option "mvs_staged": the list cost kernel takes its windows from LDS copies of the other view where they fit (default), 0 = gathers only
	bool list_rows = true;                              // option "list_rows": evaluate lists in row runs (srh_rows.hip)
	void *comm = nullptr; int comm_ranks = 0, comm_rank = 0;   // RCCL communicator (srh_comm_init)
	// bytes per band of scratch (windows, cost rows, candidate lists) the caller ASKS for: every band ends in the tails of
	// its kernels, so the largest configuration should take one band where the device has the room (MI355X: 288 GB).
	// What a run uses is band_budget(): this, capped by a share of the memory that is free right now, halved after an
	// allocation failure (budget_cap).
	size_t wbuf_budget = (size_t)32768 << 20;
	size_t budget_cap = 0;                              // 0 = none; set by with_thinner_bands after an out-of-memory run
	size_t budget_used = 0;                             // what band_budget() returned last
	size_t mem_limit = 0;                               // option "mem_limit_mb": pretend the device has only this much free (tests)
	int debug_trace = 0;                                // option "debug_trace": the list path's capacity decisions on stderr (diagnostics)
	size_t alloc_limit = 0;                             // option "debug_alloc_limit_mb": band buffers above this size are refused (tests)
	const volatile int *cancel = nullptr;
	srh_progress_fn progress = nullptr;
	void *user = nullptr;
	bool profiling = false;
	bool force_generic = false;
 	bool use_fused = false;                             // option "fused": single fused kernel for row-aligned pairs
	// option "arith": 0 = the reference's arithmetic everywhere; 3 (default) = CERTIFIED: fused multiply-adds in the strip
	// kernel's cost loops, every decision checked against an error bound, uncovered pixels redone in the reference's
	// arithmetic -- the reference's bits at the fused speed; 1 = fused multiply-adds unchecked; 2 = packed single precision
	int arith = 3;
	// srh_twoview_compute queues both passes and the cross-check and verifies the passes' counters with ONE wait at the end
	// (the plans are refuted once in a blue moon; a wait per pass leaves the GPU idle while the host launches the next one)
	// (lists: the pass took the row-run candidate lists with the capacities learnt from earlier runs -- span = the kernels'
	// maxima: longest list, most cost slots, a curve over too many rows -- to be compared with cmax / smax)
	// (guessed: the capacities were the host's first guess, estimate_list_capacity -- a pass that stands then teaches the
	// context what it measured, for reference view `ref` against `oth`)
	struct TvDefer { Counters *host = nullptr; int *span = nullptr; bool queued = false, strip = false, cert = false, lists = false, guessed = false;
	                 int cmax = 0, smax = 0, ref = -1, oth = -1; };
	TvDefer tv_defer[2];
	// ... and runs the second pass on a lane of its own (this stream, this scratch): the two passes share nothing but the
	// views, and one pass alone leaves the device idle between its kernels (~10 us each, a dozen per pass), in their tails
	// and -- the weights kernels, one wave per SIMD -- inside them
	struct TvSlot {
		hipStream_t stream = nullptr;
		hipEvent_t go = nullptr, done = nullptr;
		Scratch mem;
	} tv_slot;
	int tv_overlap = 1;                                 // option "tv_overlap": 0 = both passes on the context's stream, one after the other
	int f32_form = 0;                                   // option "f32_form" (f32 mode only, not a parity mode): 1 = the one-pass sums in single precision (priced in DESIGN.md 9.0'' (i))
	int rows_masked = 1;                                // option "rows_masked": the certified row-run cost kernel's masked blocks + single candidates: 1 = when at least 90 % of the other view's usable pixels have a fully usable window (decided on the device), 2 = always, 0 = never (a block is fast only when all 8 of its candidates are: round 5's rule)
	int side_weights = 1;                               // option "side_weights": 0 = the row-run path computes its support windows on the pass's own stream, behind the list kernel (profiling: every kernel's own duration)
	int cert_form = 1;                                  // option "cert_form": certified strip kernel in 1 = the one-pass form (default), 2 = two fused sweeps
	bool force_dense = false;                           // option "force_dense": propose the dense plan for any pinhole pair
	std::map<std::string, ProfEntry> prof;
	std::vector<PendingEvt> pending;
	srh_stats stats;
	bool last_fused = false;                            // the last TwoView pass ran the fused kernel
	int filter_invalid = 0;                             // option "filter_invalid": SRH_FILTER_* flags srh_twoview_compute ends with (0: none)
	int filter_gap_width = 2;                           // option "filter_gap_width" (GAP_WIDTH_THRESHOLD)
	int filter_replay = 0;                              // option "filter_replay": every median hole by the exact replay (test hook)
	int speckle_min_size = 0;                           // option "speckle_min_size": srh_twoview_compute* remove components below it after the cross-check (0: off)
	int speckle_diff_steps = 2;                         // option "speckle_diff_steps": that stage's max_diff in depth steps
	int cost_kind = SRH_COST_NCC;                       // option "cost": the TwoView matching cost, SRH_COST_NCC, SRH_COST_SAD or SRH_COST_CENSUS
	int sad_dense = 0;                                  // option "sad_dense": cost_sad of row-aligned rigs on the dense plan (srh_sad_strip.hip)
	int census_dense = 0;                               // option "census_dense": the census cost of row-aligned rigs on the dense plan (srh_census_strip.hip)
	int subpixel = 0;                                   // option "subpixel": every TwoView WTA pass refines its rows (srh_subpixel.hip; CHANGES RESULTS)
	// what a TwoView WTA pass keeps per reference pixel: what "wta_outputs" asks for; under "subpixel" winners and costs
	int wta_keep() const { return subpixel ? (SRH_WTA_WINNERS | SRH_WTA_COSTS) : wta_outputs; }
	int wta_outputs = 0;                                // option "wta_outputs": SRH_WTA_* planes a TwoView WTA pass keeps per reference pixel (never changes a depth map)
	// srh_mvs_fuse (srh_fuse.hip): the fused cloud of the last call -- one block carved into the arrays of
	// fuse_out -- and the call's scratch (point maps, flags, staging planes), which goes back to the pool when the call ends
	DevBuf<double> fuse_result, fuse_scratch;
	FuseCloud fuse_out = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	int64_t fuse_n = 0;
	bool fuse_valid = false;
	// where the context's own work runs, and the lists of everything a context may have in flight or hold as scratch
	Lane main_lane() { return { stream, &mem }; }
	Lane slot_lane(MvsSlot &S) { return { S.stream, S.own_buffers ? &S.mem : &mem }; }
	template <class F> void each_scratch(F f) { f(mem); f(tv_slot.mem); for (MvsSlot &S : mvs_slot) f(S.mem); }
	template <class F> void each_stream(F f) {
		for (MvsSlot &S : mvs_slot) if (S.stream) f(S.stream);
		if (side_stream) f(side_stream);
		f(stream);
		if (tv_slot.stream) f(tv_slot.stream);
	}
	void wait_streams() { each_stream([](hipStream_t s) { (void)hipStreamSynchronize(s); }); }
};

static bool cancelled(srh_context *c) { return c->cancel && *c->cancel; }
static void progress(srh_context *c, int step, const char *stage) { if (c->progress) c->progress(step, stage, c->user); }

static int drain_profile(srh_context *c) {
	for (auto &p : c->pending) {
		float ms = 0;
		HIP_TRY(hipEventSynchronize(p.b));
		HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
		ProfEntry &e = c->prof[p.name];
		e.ms += ms; e.n += 1;
		hipEventDestroy(p.a); hipEventDestroy(p.b);
	}
	c->pending.clear();
	return SRH_OK;
}

// bracket one kernel launch with events when profiling
struct Scope {
	srh_context *c; hipStream_t st; PendingEvt p; bool on;
	Scope(srh_context *c_, hipStream_t st_, const char *name, bool wanted = true) : c(c_), st(st_), on(c_->profiling && wanted) {
		if (on) {
			p.name = name;
			hipEventCreate(&p.a); hipEventCreate(&p.b);
			hipEventRecord(p.a, st);
		}
	}
	~Scope() {
		if (on) {
			hipEventRecord(p.b, st);
			c->pending.push_back(p);
			if (c->pending.size() > 4096) drain_profile(c);
		}
	}
};


static int mvs_settle_all(srh_context *c);
// settle: finish the MultiViewStereo estimates in flight first (every entry point but srh_mvs_initial_estimate itself)
static int check_slot(srh_context *c, int slot, bool must_exist, bool settle = true) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (settle) { const int rc = mvs_settle_all(c); if (rc) return rc; }
	if (slot < 0 || slot >= SRH_MAX_VIEWS) return fail(SRH_E_INVALID, "view slot %d out of range [0,%d)", slot, SRH_MAX_VIEWS);
	if (must_exist && !c->views[slot].present) return fail(SRH_E_INVALID, "view slot %d has no image", slot);
	return SRH_OK;
}

static int check_params(const srh_params *p) {
	if (!p) return fail(SRH_E_INVALID, "null params");
	if (p->num_depth_levels < 2) return fail(SRH_E_INVALID, "num_depth_levels %d < 2", p->num_depth_levels);
	if (p->window_radius < 1 || p->window_radius > 15) return fail(SRH_E_INVALID, "window_radius %d outside [1,15]", p->window_radius);
	if (!(p->image_scale > 0)) return fail(SRH_E_INVALID, "image_scale must be > 0");
	if (p->weight_kind != SRH_WEIGHT_ADAPTIVE && p->weight_kind != SRH_WEIGHT_GEODESIC)
		return fail(SRH_E_INVALID, "weight_kind %d unknown", p->weight_kind);
	return SRH_OK;
}

// ------------------------------------------------------------------ library
// srh_mvs_mrf_estimate_views keeps one stream per view busy; the HIP runtime multiplexes streams onto 4 hardware
// queues unless the process asks for more BEFORE HIP initialises (GPU_MAX_HW_QUEUES=16; measured: 8 views 277 ms
// with 4 queues, 212 with 8, 151 with 16).  The library never touches the environment: the host application sets
// the variable (bench.py and profiles/mrf_views.py do), srh_hw_queues_requested() reports what applies.
extern "C" int srh_hw_queues_requested(void) {
	const char *s = getenv("GPU_MAX_HW_QUEUES");
	const int n = s ? atoi(s) : 0;
	return n > 0 ? n : 4;                                       // the HIP runtime's default
}

extern "C" int srh_abi_version(void) { return SRH_ABI_VERSION; }
extern "C" const char *srh_build_id(void) {
	return
#include "build_id.inc"
	;
}
extern "C" const char *srh_last_error(void) { return g_err; }

extern "C" int srh_device_count(int *count) {
	if (!count) return fail(SRH_E_INVALID, "null count");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
	*count = n;
	return SRH_OK;
}

// ------------------------------------------------------------------ params / cameras (host math)
extern "C" void srh_params_twoview_defaults(srh_params *p) {
	memset(p, 0, sizeof(*p));
	p->min_depth = 10; p->max_depth = 100; p->num_depth_levels = 100;   // gui/forms/stereowidget.ui:199-288
	p->window_radius = 5;                 // twoviewstereo.cpp:66
	p->image_scale = 1.0;
	p->weight_kind = SRH_WEIGHT_GEODESIC; // twoviewstereo.cpp:84
	p->geodesic_iters = 3; p->geodesic_sigma = 50.0; p->geodesic_init = 1000000.0;   // geodesicweight.cpp:33-36,68
	p->adaptive_color_sigma = 10.0;       // adaptiveweight.cpp:26
	p->weight_cutoff = 1e-10;
	p->bad_ret = 1000; p->max_color_diff = 120;            // twoviewstereo.cpp:65,74
	p->second_best_factor = 0.95; p->wta_margin = 1e-10; p->inconsistency_thresh = 1;   // :78-79,293
	p->peak_threshold = 0.95;             // multiviewstereo.cpp:589
	p->cross_check_threshold = 1.0;
	p->neighbour_min_dot = 0.2;           // multiviewstereo.cpp:343
	p->top_k = 9; p->num_neighbours = 3;  // multiviewstereo.cpp:94,97
}

extern "C" void srh_params_mvs_defaults(srh_params *p) {
	srh_params_twoview_defaults(p);
	p->window_radius = 2;                 // multiviewstereo.cpp:91
}

// The constants of the certified arithmetic's error bound for these parameters (srh_wta.hpp, CertBound; DESIGN.md
// 2b): host arithmetic only -- what tests/test_cert_bound.py checks against an exact replay of the three arithmetics.
extern "C" int srh_cert_bound(const srh_params *p, int mvs, srh_cert_info *out) {
	if (!p || !out) return fail(SRH_E_INVALID, "null argument");
	if (p->window_radius < 1 || p->window_radius > 15) return fail(SRH_E_INVALID, "window_radius %d outside [1,15]", p->window_radius);
	const CertBound c = cert_bound(*p, mvs != 0);
	out->e0 = c.e0; out->k1 = c.k1; out->k2 = c.k2; out->k3 = c.e0 - c.room; out->zmax2 = c.zmax2; out->m_hi = c.m_hi;
	out->ok = c.ok; out->taps = (2*p->window_radius + 1)*(2*p->window_radius + 1);
	return SRH_OK;
}

extern "C" double srh_cert_sigma3(const srh_params *p, int mvs, double sum2) {
	if (!p || p->window_radius < 1 || p->window_radius > 15) return __builtin_nan("");
	return cert_bound(*p, mvs != 0).sigma3(sum2);
}

// The template scan's per-pixel bound (srh_walk.hpp: ts_pixel_setup, ts_pixel_E, ts_pixel_passes) for ONE
// pixel against ONE template pixel, host arithmetic only: the template's keep chain by the reference's own operations, its
// rooms, the pixel's bound and verdict -- what tests/test_tscan_bound_host.py holds against exact rationals.
extern "C" int srh_tscan_bound(const srh_camera *refcam, const srh_camera *othcam, const srh_params *p,
                               int tx, int ty, int x, int y, srh_tscan_bound_info *out) {
	if (!refcam || !othcam || !p || !out) return fail(SRH_E_INVALID, "null argument");
	const int D = p->num_depth_levels;
	if (D < 1 || D > 1024) return fail(SRH_E_INVALID, "num_depth_levels %d outside [1,1024]", D);
	if (refcam->is_distorted || refcam->is_refractive || othcam->is_distorted || othcam->is_refractive)
		return fail(SRH_E_UNSUPPORTED, "the template scan serves pinhole pairs");
	const double sc = p->image_scale;
	std::vector<double> tnum(D);
	double tabs = 0.0, tmn = __builtin_inf(), tmx = -__builtin_inf();
	for (int d = 0; d < D; ++d) {
		tnum[d] = pinhole_label_tnum(*refcam, *p, false, d);
		tabs = fmax(tabs, fabs(tnum[d])); tmn = fmin(tmn, tnum[d]); tmx = fmax(tmx, tnum[d]);
	}
	// the template pixel: twoview_template_kernel's keep chain
	const Ray tray = cam_unproject(*refcam, (tx + 0.5)/sc, (ty + 0.5)/sc);
	const double tnd = dot(normalized(load3(refcam->pdir)), tray.dir);
	TsRooms rooms;
	rooms.init();
	bool allproj = !(fabs(tnd) < 1e-10), chain_ok = allproj;
	double x1 = __builtin_nan(""), y1 = 0.0;
	for (int d = 0; d < D && chain_ok; ++d) {
		double x2, y2;
		if (!pinhole_project_label(tray, tnd, tnum[d], *othcam, sc, x2, y2)) { allproj = false; continue; }
		if (isnan_d(x1)) { rooms.point(x2); x1 = x2; y1 = y2; if (trunc_sat(y2) != ty) chain_ok = false; continue; }
		const double dx = x2 - x1, dy = y2 - y1;
		if (!(dx*dx + dy*dy >= 1)) { rooms.step(dx, false); continue; }
		rooms.step(dx, true); rooms.point(x2);
		if (trunc_sat(y2) != ty) chain_ok = false;
		x1 = x2; y1 = y2;
	}
	TsTemplateHdr hdr;
	const TsPixel tp = ts_pixel_setup(tray, *refcam, *othcam, sc, tabs, tmn, tmx, ty);
	ts_template_hdr(tp, rooms, allproj && chain_ok, sc, hdr);
	const Ray ray = cam_unproject(*refcam, (x + 0.5)/sc, (y + 0.5)/sc);
	const TsPixel pp = ts_pixel_setup(ray, *refcam, *othcam, sc, tabs, tmn, tmx, y);
	const double E = pp.ok ? ts_pixel_E(pp, hdr, sc, (double)(x - tx)) : __builtin_inf();
	out->E = E; out->eU = pp.eU; out->eU_template = hdr.eU; out->dyU = pp.dyU;
	out->room_col = hdr.room_col; out->room_one = hdr.room_one; out->room_proj = hdr.room_proj;
	out->pixel_ok = pp.ok ? 1 : 0; out->template_ok = hdr.ok;
	out->passes = ts_pixel_passes(pp, hdr, E) ? 1 : 0; out->pad_ = 0;
	return SRH_OK;
}

static bool near_zero(double x) { return (x <= 1e-10 && x >= -1e-10); }   // camera.cpp:51-52

extern "C" int srh_camera_from_krt(const double K[9], const double Rin[9], const double t[3],
                                   const double dist[5], const double plane_normal[3],
                                   double plane_dist, double refr_index, srh_camera *out)
{
	if (!K || !Rin || !t || !out) return fail(SRH_E_INVALID, "null argument");
	srh_camera c;
	memset(&c, 0, sizeof(c));
	memcpy(c.K, K, sizeof(c.K));
	memcpy(c.R, Rin, sizeof(c.R));
	memcpy(c.t, t, sizeof(c.t));
	// orthonormalize(R_): Gram-Schmidt over columns, then flush |v| < 1e-10 to 0 (camera.cpp:140-160)
	for (int i = 0; i < 3; ++i) {
		Vec3 accum = v3(0, 0, 0);
		for (int j = 0; j < i; ++j) {
			const Vec3 vi = v3(c.R[i], c.R[3 + i], c.R[6 + i]);
			const Vec3 vj = v3(c.R[j], c.R[3 + j], c.R[6 + j]);
			const double scale = dot(vi, vj) / dot(vj, vj);
			accum = accum + vj*scale;
		}
		const Vec3 col = normalized(v3(c.R[i], c.R[3 + i], c.R[6 + i]) - accum);
		c.R[i] = col.x; c.R[3 + i] = col.y; c.R[6 + i] = col.z;
	}
	for (int k = 0; k < 9; ++k) if (-1e-10 < c.R[k] && c.R[k] < 1e-10) c.R[k] = 0.0;
	{   // Kinv_ = K_.inverse() (3x3 cofactor inverse)
		const double *m = c.K;
		const double c00 = m[4]*m[8] - m[5]*m[7];
		const double c01 = m[5]*m[6] - m[3]*m[8];
		const double c02 = m[3]*m[7] - m[4]*m[6];
		const double det = (m[0]*c00 + m[1]*c01) + m[2]*c02;
		const double invdet = 1.0 / det;
		c.Kinv[0] = c00*invdet;
		c.Kinv[1] = (m[2]*m[7] - m[1]*m[8])*invdet;
		c.Kinv[2] = (m[1]*m[5] - m[2]*m[4])*invdet;
		c.Kinv[3] = c01*invdet;
		c.Kinv[4] = (m[0]*m[8] - m[2]*m[6])*invdet;
		c.Kinv[5] = (m[2]*m[3] - m[0]*m[5])*invdet;
		c.Kinv[6] = c02*invdet;
		c.Kinv[7] = (m[1]*m[6] - m[0]*m[7])*invdet;
		c.Kinv[8] = (m[0]*m[4] - m[1]*m[3])*invdet;
	}
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) c.Rinv[i*3 + j] = c.R[j*3 + i];
	{ const Vec3 C = matvec(c.Rinv, v3(-t[0], -t[1], -t[2])); c.C[0] = C.x; c.C[1] = C.y; c.C[2] = C.z; }
	{   // updatePrincipleRay (camera.cpp:292-298)
		const Vec3 tc = v3(c.K[2]/c.K[8], c.K[5]/c.K[8], c.K[8]/c.K[8]);
		const Vec3 dir = normalized(matvec(c.Kinv, tc));
		const Vec3 pd = normalized(matvec(c.Rinv, dir));
		c.pdir[0] = pd.x; c.pdir[1] = pd.y; c.pdir[2] = pd.z;
	}
	if (dist) {
		memcpy(c.dist, dist, sizeof(c.dist));
		c.is_distorted = !near_zero(dist[0]) || !near_zero(dist[1]) || !near_zero(dist[2])
		              || !near_zero(dist[3]) || !near_zero(dist[4]);
	}
	c.plane_normal[2] = 1.0; c.plane_dist = 0.0; c.refr_index = 1.0;
	if (plane_normal) {
		const Vec3 n = normalized(load3(plane_normal));       // Plane3d ctor, plane.hpp:32
		c.plane_normal[0] = n.x; c.plane_normal[1] = n.y; c.plane_normal[2] = n.z;
		c.plane_dist = plane_dist;
		c.refr_index = refr_index;
	}
	c.is_refractive = (!near_zero(c.refr_index - 1) && !near_zero(c.plane_dist));   // camera.cpp:326-344
	*out = c;
	return SRH_OK;
}

extern "C" int srh_camera_from_p(const double Pin[12], const double dist[5], const double plane_normal[3],
                                 double plane_dist, double refr_index, srh_camera *out)
{
	if (!Pin || !out) return fail(SRH_E_INVALID, "null argument");
	// Camera::updateOthers (camera.cpp:251-288)
	const double n2 = (Pin[8]*Pin[8] + Pin[9]*Pin[9]) + Pin[10]*Pin[10];
	if (!(n2 > 0)) return fail(SRH_E_INVALID, "projection matrix with a zero third row");
	double P[3][4];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) P[i][j] = Pin[i*4 + j] / n2;
	// A = (reverseRows * M)^T, Householder QR (Eigen::HouseholderQR, unblocked): A = Q * Rt
	double A[3][3], tau[3];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = P[2 - j][i];
	for (int k = 0; k < 3; ++k) {
		const double c0 = A[k][k];
		double tailSq = 0;
		for (int i = k + 1; i < 3; ++i) tailSq += A[i][k]*A[i][k];
		double beta;
		if (tailSq <= std::numeric_limits<double>::min()) {       // makeHouseholder: nothing to annihilate
			tau[k] = 0; beta = c0;
			for (int i = k + 1; i < 3; ++i) A[i][k] = 0;
		} else {
			beta = sqrt(c0*c0 + tailSq);
			if (c0 >= 0) beta = -beta;
			for (int i = k + 1; i < 3; ++i) A[i][k] /= (c0 - beta);   // essential part, stored below the diagonal
			tau[k] = (beta - c0)/beta;
		}
		A[k][k] = beta;
		for (int j = k + 1; j < 3; ++j) {                             // H_k applied to the remaining columns
			double tmp = 0;
			for (int i = k + 1; i < 3; ++i) tmp += A[i][k]*A[i][j];
			tmp += A[k][j];
			A[k][j] -= tau[k]*tmp;
			for (int i = k + 1; i < 3; ++i) A[i][j] -= tau[k]*A[i][k]*tmp;
		}
	}
	double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
	for (int k = 2; k >= 0; --k)                                     // householderQ(): H0 H1 H2
		for (int j = k; j < 3; ++j) {
			double tmp = 0;
			for (int i = k + 1; i < 3; ++i) tmp += A[i][k]*Q[i][j];
			tmp += Q[k][j];
			Q[k][j] -= tau[k]*tmp;
			for (int i = k + 1; i < 3; ++i) Q[i][j] -= tau[k]*A[i][k]*tmp;
		}
	double K[9], R[9];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			R[i*3 + j] = Q[j][2 - i];                                  // reverseRows * Q^T
			K[i*3 + j] = (2 - j <= 2 - i) ? A[2 - j][2 - i] : 0.0;     // reverseRows * Rt^T * reverseRows
		}
	for (int axis = 2; axis >= 0; --axis) {                          // positive diagonal of K (camera.cpp:266-275)
		if (K[axis*3 + axis] < 0) {
			K[axis*3 + axis] = -K[axis*3 + axis];
			for (int j = 0; j < 3; ++j) R[axis*3 + j] = -R[axis*3 + j];
		}
		if (K[axis*3 + 2] < 0) K[axis*3 + 2] = -K[axis*3 + 2];
	}
	// t_ = Kinv_ * P_.col(3): Kinv is the cofactor inverse srh_camera_from_krt computes again below
	srh_camera tmpc;
	const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
	int rc = srh_camera_from_krt(K, I3, z3, nullptr, nullptr, 0.0, 1.0, &tmpc);
	if (rc) return rc;
	const Vec3 t = matvec(tmpc.Kinv, v3(P[0][3], P[1][3], P[2][3]));
	const double tt[3] = { t.x, t.y, t.z };
	return srh_camera_from_krt(K, R, tt, dist, plane_normal, plane_dist, refr_index, out);
}

extern "C" int srh_mvs_neighbours(int nviews, const srh_camera *cams, const srh_params *p,
                                  int32_t *neigh, int32_t *count)
{
	if (nviews < 0 || !cams || !p || !neigh || !count) return fail(SRH_E_INVALID, "null argument");
	if (p->num_neighbours < 0) return fail(SRH_E_INVALID, "num_neighbours < 0");
	// multiviewstereo.cpp:335-360
	for (int v = 0; v < nviews; ++v) {
		std::vector<std::pair<double, int>> nearViews;
		for (int v2 = 0; v2 < nviews; ++v2) {
			if (v == v2) continue;
			if (fabs(dot(load3(cams[v].pdir), load3(cams[v2].pdir))) > p->neighbour_min_dot) {
				const Vec3 d = load3(cams[v].C) - load3(cams[v2].C);
				nearViews.push_back(std::make_pair(dot(d, d), v2));
			}
		}
		size_t end = nearViews.size();
		if ((size_t)p->num_neighbours < nearViews.size()) {
			std::sort(nearViews.begin(), nearViews.end());
			end = (size_t)p->num_neighbours;
		}
		for (size_t k = 0; k < end; ++k) neigh[(size_t)v*p->num_neighbours + k] = nearViews[k].second;
		count[v] = (int32_t)end;
	}
	return SRH_OK;
}

// ------------------------------------------------------------------ context
extern "C" int srh_create(int device, srh_context **out) {
	if (!out) return fail(SRH_E_INVALID, "null out");
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) {
		(void)hipGetLastError();
		return fail(SRH_E_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
		            e != hipSuccess ? hipGetErrorString(e) : "device count 0");
	}
	if (device < 0 || device >= n) return fail(SRH_E_INVALID, "device ordinal %d outside [0,%d)", device, n);
	HIP_TRY(hipSetDevice(device));
	srh_context *c = new srh_context();
	c->device = device;
	memset(&c->stats, 0, sizeof(c->stats));
	// (no environment overrides: which arithmetic / path a host runs is decided by srh_set_option alone, and reported
	// by srh_get_stats; bench.py maps its own SRH_BENCH_* variables to options)
	{ int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus; }
	hipError_t e2 = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
	if (e2 != hipSuccess) { delete c; return fail(SRH_E_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e2)); }
	c->stream = c->own_stream;
	if (c->d_views.alloc(SRH_MAX_VIEWS) != hipSuccess || c->d_slots.alloc(SRH_MAX_VIEWS) != hipSuccess ||
	    c->mem.cnt.alloc(1) != hipSuccess || c->mem.span.alloc(4) != hipSuccess) {
		srh_destroy(c);
		return fail(SRH_E_DEVICE, "allocating the context tables failed");
	}
	// ordered on the context's own (non-blocking) stream, which the null stream does not synchronise with
	if (hipMemsetAsync(c->d_views, 0, sizeof(ViewDev)*SRH_MAX_VIEWS, c->stream) != hipSuccess ||
	    hipMemsetAsync(c->mem.cnt, 0, sizeof(Counters), c->stream) != hipSuccess ||
	    hipStreamSynchronize(c->stream) != hipSuccess) {
		srh_destroy(c);
		return fail(SRH_E_DEVICE, "initialising the context tables failed");
	}
	*out = c;
	return SRH_OK;
}

// (freeing a plane used to wait for the device; so does this, before a plane can reach another context)
static void free_view(ViewHost &v) {
	if (v.rgba || v.gray || v.edges || v.tvp || v.geo5) (void)hipDeviceSynchronize();
	v.rgba.release(); v.mask.release(); v.gray.release(); v.gray_tv.release(); v.depth.release(); v.edges.release();
	v.full.release(); v.fulls.release(); v.census.release(); v.cenothp.release(); v.cenrefp.release(); v.grayp.release(); v.fullsp.release(); v.tvp.release(); v.geo5.release(); v.fullp.release(); v.act.release(); v.peaks.release(); v.mrf.release(); v.sgm.release();
	v.wta_xy.release(); v.wta_cost.release();
	v.subpx_delta.release(); v.subpx_neigh.release(); v.subpx_cls.release();
	v = ViewHost();
}

extern "C" void srh_destroy(srh_context *c) {
	if (!c) return;
	hipSetDevice(c->device);
	if (c->own_stream) hipStreamSynchronize(c->own_stream);
	if (c->stream) c->wait_streams();
	for (MvsSlot &S : c->mvs_slot) S.pending = false;
	if (c->side_stream) hipStreamDestroy(c->side_stream);
	if (c->side_go) hipEventDestroy(c->side_go);
	if (c->side_done) hipEventDestroy(c->side_done);
	if (c->side_tpl) hipEventDestroy(c->side_tpl);
	drain_profile(c);
	for (MvsSlot &S : c->mvs_slot) {
		if (S.stream) hipStreamDestroy(S.stream);
		if (S.ev) hipEventDestroy(S.ev);
		if (S.done) hipEventDestroy(S.done);
		if (S.h_maxc) hipHostFree(S.h_maxc);
	}
	for (auto &v : c->views) free_view(v);
	c->d_views.release(); c->d_slots.release();
	// (every stream of the context has been waited for above: its scratch is idle and goes to the process's pool)
	(void)hipDeviceSynchronize();
	c->each_scratch([](Scratch &m) { m.release(); });
	for (auto &d : c->tv_defer) { if (d.host) hipHostFree(d.host); if (d.span) hipHostFree(d.span); }
	{
		srh_context::TvSlot &T = c->tv_slot;
		if (T.stream) hipStreamDestroy(T.stream);
		if (T.go) hipEventDestroy(T.go);
		if (T.done) hipEventDestroy(T.done);
	}
	c->mrf_peaks.release();
	c->mvs_subpx.release();
	for (LabelStage *S : c->label_stages) S->release();
	c->fuse_result.release(); c->fuse_scratch.release();
	for (int i = 0; i < SRH_MAX_VIEWS; ++i) if (c->mrf_stream[i]) hipStreamDestroy(c->mrf_stream[i]);
	if (c->views_go) hipEventDestroy(c->views_go);
	if (c->mrf_host) hipHostFree(c->mrf_host);
	if (c->mvsgm_host) hipHostFree(c->mvsgm_host);
	if (c->comm) (void)rccl_comm_destroy(c->comm);
	if (c->own_stream) hipStreamDestroy(c->own_stream);
	delete c;
}

extern "C" int srh_set_stream(srh_context *c, void *hip_stream) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	{ const int rc = mvs_settle_all(c); if (rc) return rc; }
	c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
	return SRH_OK;
}

extern "C" int srh_set_hooks(srh_context *c, const volatile int *cancel, srh_progress_fn progress_fn, void *user) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	c->cancel = cancel; c->progress = progress_fn; c->user = user;
	return SRH_OK;
}

static void release_band_buffers(srh_context *c);

extern "C" int srh_set_option(srh_context *c, const char *name, long value) {
	if (!c || !name) return fail(SRH_E_INVALID, "null argument");
	{ const int rc = mvs_settle_all(c); if (rc) return rc; }       // options apply to work queued from here on
	if (!strcmp(name, "list_rows")) { c->list_rows = value != 0; return SRH_OK; }
	if (!strcmp(name, "list_count_pass")) { c->list_count_pass = value != 0; return SRH_OK; }
	if (!strcmp(name, "force_generic")) { c->force_generic = value != 0; c->force_walk = value == 2; return SRH_OK; }
	if (!strcmp(name, "fused")) { c->use_fused = value != 0; return SRH_OK; }
	if (!strcmp(name, "arith")) {
		if (value < 0 || value > 3) return fail(SRH_E_INVALID, "arith must be 0 (exact), 1 (fma), 2 (f32) or 3 (certified fma)");
		c->arith = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "force_dense")) { c->force_dense = value != 0; return SRH_OK; }
	if (!strcmp(name, "cert_form")) {
		if (value != 1 && value != 2) return fail(SRH_E_INVALID, "cert_form must be 1 (one-pass) or 2 (two fused sweeps)");
		c->cert_form = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "strip")) {
		if (value != 0 && value != 1 && value != 4 && value != 8) return fail(SRH_E_INVALID, "strip must be 0, 1, 4 or 8");
		c->strip = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "mvs_staged")) { c->mvs_staged = value != 0; return SRH_OK; }
	if (!strcmp(name, "mvs_async")) { c->mvs_async = value != 0; return SRH_OK; }
	if (!strcmp(name, "band_budget_mb")) {
		if (value < 1) return fail(SRH_E_INVALID, "band_budget_mb must be >= 1");
		c->wbuf_budget = (size_t)value << 20;
		c->budget_cap = 0;                                         // a new request: earlier out-of-memory halvings are forgotten
		return SRH_OK;
	}
	// tests of the budget logic: pretend the device has only `value` MB to give / refuse band buffers above `value` MB
	if (!strcmp(name, "mem_limit_mb")) { c->mem_limit = value > 0 ? (size_t)value << 20 : 0; return SRH_OK; }
	if (!strcmp(name, "debug_trace")) { c->debug_trace = (int)value; return SRH_OK; }
	if (!strcmp(name, "band_pool_mb")) {
		// process-wide: how many bytes of released band buffers wait for the next context (0: none, and what waits now is freed)
		if (value < 0) return fail(SRH_E_INVALID, "band_pool_mb must be >= 0");
		{ std::lock_guard<std::mutex> g(g_pool_mu); g_pool_cap = (size_t)value << 20; }
		if (value == 0) pool_flush(-1);
		return SRH_OK;
	}
	if (!strcmp(name, "debug_alloc_limit_mb")) {
		c->alloc_limit = g_alloc_limit = value > 0 ? (size_t)value << 20 : 0;
		// the band buffers a bigger run left behind would serve every later request without an allocation: start afresh
		c->wait_streams();
		release_band_buffers(c);
		return SRH_OK;
	}
	if (!strcmp(name, "tv_overlap")) { c->tv_overlap = value != 0; return SRH_OK; }
	if (!strcmp(name, "filter_invalid")) {
		if (value < 0 || value > 3) return fail(SRH_E_INVALID, "filter_invalid must be 0..3 (SRH_FILTER_GAPS | SRH_FILTER_MEDIAN)");
		c->filter_invalid = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "filter_gap_width")) { c->filter_gap_width = (int)value; return SRH_OK; }
	if (!strcmp(name, "filter_replay")) { c->filter_replay = value != 0; return SRH_OK; }
	if (!strcmp(name, "speckle_min_size")) {
		if (value < 0 || value > INT32_MAX) return fail(SRH_E_INVALID, "speckle_min_size must be in [0, 2^31)");
		c->speckle_min_size = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "speckle_diff_steps")) {
		if (value < 1 || value > INT32_MAX) return fail(SRH_E_INVALID, "speckle_diff_steps must be >= 1");
		c->speckle_diff_steps = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "cost")) {
		if (value != SRH_COST_NCC && value != SRH_COST_SAD && value != SRH_COST_CENSUS)
			return fail(SRH_E_INVALID, "cost must be 0 (SRH_COST_NCC), 1 (SRH_COST_SAD) or 3 (SRH_COST_CENSUS)");
		c->cost_kind = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "sad_dense")) { c->sad_dense = value != 0; return SRH_OK; }
	if (!strcmp(name, "census_dense")) { c->census_dense = value != 0; return SRH_OK; }
	if (!strcmp(name, "wta_outputs")) {
		if (value != 0 && value != SRH_WTA_WINNERS && value != (SRH_WTA_WINNERS | SRH_WTA_COSTS))
			return fail(SRH_E_INVALID, "wta_outputs must be 0, 1 (SRH_WTA_WINNERS) or 3 (SRH_WTA_WINNERS | SRH_WTA_COSTS): the costs are those of the kept winners");
		c->wta_outputs = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "subpixel")) {
		if (value != 0 && value != 1) return fail(SRH_E_INVALID, "subpixel must be 0 or 1");
		c->subpixel = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "mvs_subpixel_search")) {
		if (value != 0 && value != 1) return fail(SRH_E_INVALID, "mvs_subpixel_search must be 0 or 1");
		c->mvs_subpx_search = (int)value; return SRH_OK;
	}
	if (!strcmp(name, "tscan")) { c->tscan = value != 0; return SRH_OK; }
	if (!strcmp(name, "tscan_bound")) { c->tscan_bound = value != 0; return SRH_OK; }
	if (!strcmp(name, "geodma")) { c->geodma = value != 0; return SRH_OK; }
	if (!strcmp(name, "f32_form")) { c->f32_form = value != 0; return SRH_OK; }
	if (!strcmp(name, "rows_masked")) { c->rows_masked = (int)value; return SRH_OK; }   // 0 off, 1 by the other view's share of fully usable windows (default), 2 always
	if (!strcmp(name, "side_weights")) { c->side_weights = value != 0; return SRH_OK; }
	// test of the cut-list redo: the capacity the next MultiViewStereo estimate is queued with (0 = forget what was learnt)
	if (!strcmp(name, "debug_mvs_cmax_hint")) { c->mvs_cmax_hint = value > 0 ? (int)((value + 7) & ~7L) : 0; return SRH_OK; }
#ifdef SRH_EXPERIMENT
	if (!strcmp(name, "exp_repeat")) { exp_set((int)value, -1); return SRH_OK; }
	if (!strcmp(name, "exp_lds_pad")) { exp_set(-1, (int)value); return SRH_OK; }
	if (!strcmp(name, "exp_scan_mode")) { exp_set_scan((int)value); return SRH_OK; }
	if (!strcmp(name, "exp_walk_mode")) { exp_set_walk((int)value); return SRH_OK; }
	if (!strcmp(name, "exp_rows_mode")) { exp_set_rows((int)value); return SRH_OK; }
#endif
	return fail(SRH_E_INVALID, "unknown option '%s'", name);
}

extern "C" int srh_synchronize(srh_context *c) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	HIP_TRY(hipSetDevice(c->device));
	{ const int rc = mvs_settle_all(c); if (rc) return rc; }
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// ------------------------------------------------------------------ views
// The pixels and mask of a w x h view into `slot` and every plane derived from them.  rgba / mask: host memory
// (srh_view_upload) or device memory of this context's device (srh_view_upload_scaled), as `kind` says; hmask: the mask
// bytes in host memory (null with a null mask).
static int view_install(srh_context *c, int slot, int w, int h, const void *rgba, const void *mask, const uint8_t *hmask,
                        hipMemcpyKind kind, const srh_camera *cam)
{
	if (w <= 0 || h <= 0 || (size_t)w*h > ((size_t)1 << 30)) return fail(SRH_E_INVALID, "bad image size %dx%d", w, h);
	if (!rgba || !cam) return fail(SRH_E_INVALID, "null rgba / camera");
	// (before anything is allocated or launched: the slot keeps what it held)
	if (w > SRH_MAX_VIEW_DIM || h > SRH_MAX_VIEW_DIM) return fail(SRH_E_UNSUPPORTED, "view of %dx%d: a side above %d (SRH_MAX_VIEW_DIM)", w, h, SRH_MAX_VIEW_DIM);
	HIP_TRY(hipSetDevice(c->device));
	ViewHost &v = c->views[slot];
	const size_t n = (size_t)w*h;
	if (!v.present || v.w != w || v.h != h) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		free_view(v);
		HIP_TRY(v.rgba.alloc(n));
		HIP_TRY(v.mask.alloc(n));
		HIP_TRY(v.gray.alloc(n));
		HIP_TRY(v.gray_tv.alloc(n));
		HIP_TRY(v.depth.alloc(n));
		HIP_TRY(v.edges.alloc(4*n));
		HIP_TRY(v.full.alloc(full_stat_offset(n) + 16));      // (+ the map's two counters, full_window_kernel)
		v.w = w; v.h = h; v.present = true;
	}
	v.cam = *cam;
	v.full_r = 0; v.fulls_r = 0;                                // recomputed on demand for the new pixels
	v.tvp_valid = false; v.fullp_r = 0; v.grayp_valid = false; v.census_valid = false; v.cenp_valid = false; v.fullsp_r = 0; v.geo5_valid = false; v.geo5_denied = false;
	v.peaks_k = 0;                                              // the top-K peaks belonged to the previous image
	v.wta_flags = 0; v.wta_oth = -1;                            // and so did the WTA by-products
	for (LabelStage *S : c->label_stages) S->forget_if(w, h);   // and so may what a label stage reports
	for (int j = 0; j < SRH_MAX_VIEWS; ++j) { v.list_mode[j] = 0; c->views[j].list_mode[slot] = 0; }   // new geometry
	HIP_TRY(hipMemcpyAsync(v.rgba, rgba, n*4, kind, c->stream));
	if (mask) HIP_TRY(hipMemcpyAsync(v.mask, mask, n, kind, c->stream));
	else      HIP_TRY(hipMemsetAsync(v.mask, 1, n, c->stream));
	if (mask) v.hmask.assign(hmask, hmask + n); else v.hmask.clear();
	v.act_valid = false;
	{ Scope s(c, c->stream, "prep_view_kernel"); launch_prep_view(c->stream, v.rgba, v.mask, w, h, v.gray, v.gray_tv); }
	{ Scope s(c, c->stream, "edge_planes_kernel"); launch_edge_planes(c->stream, v.rgba, w, h, v.edges); }
	launch_fill(c->stream, v.depth, n, __builtin_nan(""));
	ViewDev d;
	d.w = w; d.h = h; d.rgba = v.rgba; d.mask = v.mask; d.gray = v.gray; d.gray_tv = v.gray_tv; d.depth = v.depth;
	d.cam = v.cam;
	d.census = v.census;                                        // (null, or a plane of this size that ensure_census refills)
	HIP_TRY(hipMemcpyAsync(c->d_views + slot, &d, sizeof(d), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));   // the host buffers and `d` may go away after return
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

extern "C" int srh_view_upload(srh_context *c, int slot, int w, int h,
                               const uint8_t *rgba, const uint8_t *mask, const srh_camera *cam)
{
	int rc = check_slot(c, slot, false); if (rc) return rc;
	return view_install(c, slot, w, h, rgba, mask, mask, hipMemcpyHostToDevice, cam);
}

// ---- views at file resolution: Qt's scaling on the device (srh_scale.hip)
extern "C" int srh_scaled_size(int src_w, int src_h, double image_scale, int mode, int *w_out, int *h_out) {
	int w = 0, h = 0;
	const char *why = "";
	const int rc = scale_target_size(src_w, src_h, image_scale, mode, &w, &h, &why);
	if (rc) return fail(rc, "%dx%d at scale %g: %s", src_w, src_h, image_scale, why);
	if (w_out) *w_out = w;
	if (h_out) *h_out = h;
	return SRH_OK;
}

// The staging of one scaling: the source image at file resolution and the fast scale's index maps.  Blocks of the view
// planes' allocator; release() once the stream has drained (the kernels queued on it read them).
struct ScaleStage {
	DevBuf<uint32_t> src;
	DevBuf<int32_t> dmap;
	std::vector<int32_t> hmap;                                        // the maps on the host: alive until the copy queued from it is done
	void release() { src.release(); dmap.release(); }
};

static int stage_source(srh_context *c, const uint8_t *rgba, int sw, int sh, ScaleStage &st) {
	const size_t ns = (size_t)sw*sh;
	if (ns > ((size_t)1 << 30)) return fail(SRH_E_INVALID, "bad image size %dx%d", sw, sh);
	HIP_TRY(st.src.alloc(ns + 4));                                     // (+ the reach of the smooth kernel's aligned 16-byte loads)
	HIP_TRY(hipMemsetAsync(st.src + ns, 0, 16, c->stream));
	HIP_TRY(hipMemcpyAsync(st.src, rgba, ns*4, hipMemcpyHostToDevice, c->stream));
	return SRH_OK;
}

// The staged sw x sh source scaled to dw x dh (scale_target_size's answer, not the identity) into `out`, a device buffer the
// caller releases; queued on the context's stream.  The smooth scale premultiplies the staged source in place: a fast scale
// of the same source is queued before it.
static int scale_staged(srh_context *c, ScaleStage &st, int sw, int sh, bool has_alpha, int dw, int dh, int mode, DevBuf<uint32_t> &out) {
	const size_t ns = (size_t)sw*sh;
	if (mode == SRH_SCALE_SMOOTH) {
		if (!(scale_axis_inside(sw, dw) && scale_axis_inside(sh, dh)))
			return fail(SRH_E_UNSUPPORTED, "%dx%d -> %dx%d: a run of the smooth scale would leave the image", sw, sh, dw, dh);
		HIP_TRY(out.alloc((size_t)dw*dh));
		{ Scope s(c, c->stream, "premultiply_kernel"); launch_premultiply(c->stream, st.src, ns, has_alpha); }
		{ Scope s(c, c->stream, "smooth_scale_kernel"); launch_smooth_scale(c->stream, st.src, sw, sh, out, dw, dh); }
	} else {
		std::vector<int32_t> &map = st.hmap;
		map.assign((size_t)dw + dh, 0);
		if (!scale_fast_maps(sw, sh, dw, dh, has_alpha, map.data()))
			return fail(SRH_E_UNSUPPORTED, "%dx%d -> %dx%d: a tap of the fast scale would leave the image", sw, sh, dw, dh);
		HIP_TRY(out.alloc((size_t)dw*dh));
		HIP_TRY(st.dmap.alloc(map.size()));
		HIP_TRY(hipMemcpyAsync(st.dmap, map.data(), map.size()*sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
		{ Scope s(c, c->stream, "fast_scale_kernel"); launch_fast_scale(c->stream, st.src, sw, out, dw, dh, st.dmap, has_alpha); }
	}
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

// the identity (dw == sw): the staged source itself becomes `out`; an opaque source gets alpha 255
static int scale_identity(srh_context *c, ScaleStage &st, int sw, int sh, bool has_alpha, DevBuf<uint32_t> &out) {
	if (!has_alpha) { Scope s(c, c->stream, "premultiply_kernel"); launch_premultiply(c->stream, st.src, (size_t)sw*sh, false); }
	out = std::move(st.src);
	return SRH_OK;
}

// the stream drained, the staging back in the pool; rc, or the device's error
static int scale_finish(srh_context *c, ScaleStage &st, int rc) {
	const hipError_t e = hipStreamSynchronize(c->stream);
	st.release();
	if (rc == SRH_OK && e != hipSuccess) rc = fail(SRH_E_DEVICE, "image scaling: %s", hipGetErrorString(e));
	return rc;
}

extern "C" int srh_image_scale(srh_context *c, const uint8_t *rgba, int src_w, int src_h, int has_alpha, double image_scale, int mode,
                               uint8_t *rgba_out, int *w_out, int *h_out)
{
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (!rgba || !rgba_out) return fail(SRH_E_INVALID, "null rgba");
	int dw = 0, dh = 0;
	int rc = srh_scaled_size(src_w, src_h, image_scale, mode, &dw, &dh); if (rc) return rc;
	{ rc = mvs_settle_all(c); if (rc) return rc; }
	HIP_TRY(hipSetDevice(c->device));
	ScaleStage st;
	DevBuf<uint32_t> out;
	rc = stage_source(c, rgba, src_w, src_h, st);
	if (rc == SRH_OK) rc = dw == src_w ? scale_identity(c, st, src_w, src_h, has_alpha != 0, out)
	                                   : scale_staged(c, st, src_w, src_h, has_alpha != 0, dw, dh, mode, out);
	rc = scale_finish(c, st, rc);
	if (rc == SRH_OK) {
		const hipError_t e = hipMemcpy(rgba_out, out, (size_t)dw*dh*4, hipMemcpyDeviceToHost);
		if (e != hipSuccess) rc = fail(SRH_E_DEVICE, "image scaling, read-back: %s", hipGetErrorString(e));
	}
	out.release();
	if (rc) return rc;
	if (w_out) *w_out = dw;
	if (h_out) *h_out = dh;
	return SRH_OK;
}

extern "C" int srh_view_upload_scaled(srh_context *c, int slot, int src_w, int src_h, const uint8_t *rgba, int has_alpha,
                                      const uint8_t *mask_rgba, int mask_w, int mask_h, int mask_has_alpha,
                                      double image_scale, int mask_rule, const srh_camera *cam)
{
	int rc = check_slot(c, slot, false); if (rc) return rc;
	if (!rgba || !cam) return fail(SRH_E_INVALID, "null rgba / camera");
	if (mask_rule != SRH_MASK_NONE && mask_rule != SRH_MASK_ALPHA_FAST && mask_rule != SRH_MASK_IMAGE_SMOOTH)
		return fail(SRH_E_INVALID, "mask_rule %d unknown", mask_rule);
	// every refusal of a shape comes before the slot is touched
	int dw = 0, dh = 0, mw = 0, mh = 0;
	if ((rc = srh_scaled_size(src_w, src_h, image_scale, SRH_SCALE_SMOOTH, &dw, &dh))) return rc;
	if (dw > SRH_MAX_VIEW_DIM || dh > SRH_MAX_VIEW_DIM)
		return fail(SRH_E_UNSUPPORTED, "%dx%d at scale %g: a view of %dx%d, a side above %d (SRH_MAX_VIEW_DIM)", src_w, src_h, image_scale, dw, dh, SRH_MAX_VIEW_DIM);
	const bool alpha_mask = mask_rule == SRH_MASK_ALPHA_FAST && has_alpha;
	const bool image_mask = mask_rule == SRH_MASK_IMAGE_SMOOTH && mask_rgba;
	if (alpha_mask && (rc = srh_scaled_size(src_w, src_h, image_scale, SRH_SCALE_FAST, &mw, &mh))) return rc;
	if (image_mask && (rc = srh_scaled_size(mask_w, mask_h, image_scale, SRH_SCALE_SMOOTH, &mw, &mh))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	ScaleStage st, mst;
	DevBuf<uint32_t> img, mimg;
	DevBuf<uint8_t> dmask;
	std::vector<uint8_t> hmask;
	const bool identity = dw == src_w;
	auto run = [&]() -> int {
		// the image is staged once: the mask source of MultiViewStereo's rule is its fast scale, queued before the smooth
		// scale premultiplies the staging in place
		int r = stage_source(c, rgba, src_w, src_h, st); if (r) return r;
		if (alpha_mask && !identity && (r = scale_staged(c, st, src_w, src_h, true, mw, mh, SRH_SCALE_FAST, mimg))) return r;
		r = identity ? scale_identity(c, st, src_w, src_h, has_alpha != 0, img)
		             : scale_staged(c, st, src_w, src_h, has_alpha != 0, dw, dh, SRH_SCALE_SMOOTH, img);
		if (r) return r;
		if (image_mask) {
			if ((r = stage_source(c, mask_rgba, mask_w, mask_h, mst))) return r;
			r = mw == mask_w ? scale_identity(c, mst, mask_w, mask_h, mask_has_alpha != 0, mimg)
			                 : scale_staged(c, mst, mask_w, mask_h, mask_has_alpha != 0, mw, mh, SRH_SCALE_SMOOTH, mimg);
			if (r) return r;
		}
		if (alpha_mask || image_mask) {
			const size_t n = (size_t)dw*dh;
			HIP_TRY(dmask.alloc(n));
			// (the identity under MultiViewStereo's rule: the fast copy is the image itself)
			const uint32_t *msrc = alpha_mask && identity ? img.p : mimg.p;
			{ Scope s(c, c->stream, "scale_mask_kernel"); launch_scale_mask(c->stream, msrc, mw, mh, alpha_mask, dmask, dw, dh); }
			hmask.resize(n);
			HIP_TRY(hipMemcpyAsync(hmask.data(), dmask, n, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
		}
		return view_install(c, slot, dw, dh, img, dmask.p, hmask.data(), hipMemcpyDeviceToDevice, cam);
	};
	rc = run();
	rc = scale_finish(c, st, rc);
	mst.release(); img.release(); mimg.release(); dmask.release();
	return rc;
}

extern "C" int srh_view_image_download(srh_context *c, int slot, uint8_t *rgba_out, uint8_t *mask_out) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	if (rgba_out) HIP_TRY(hipMemcpyAsync(rgba_out, v.rgba, n*4, hipMemcpyDeviceToHost, c->stream));
	if (mask_out) HIP_TRY(hipMemcpyAsync(mask_out, v.mask, n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

extern "C" int srh_view_size(srh_context *c, int slot, int *w, int *h) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (w) *w = c->views[slot].w;
	if (h) *h = c->views[slot].h;
	return SRH_OK;
}

extern "C" int srh_view_depth_download(srh_context *c, int slot, double *host_out) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!host_out) return fail(SRH_E_INVALID, "null output");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	HIP_TRY(hipMemcpyAsync(host_out, v.depth, (size_t)v.w*v.h*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

extern "C" int srh_view_depth_upload(srh_context *c, int slot, const double *host_in) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!host_in) return fail(SRH_E_INVALID, "null input");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	HIP_TRY(hipMemcpyAsync(v.depth, host_in, (size_t)v.w*v.h*sizeof(double), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

extern "C" int srh_view_depth_device_ptr(srh_context *c, int slot, void **dev_ptr) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!dev_ptr) return fail(SRH_E_INVALID, "null output");
	*dev_ptr = c->views[slot].depth;
	return SRH_OK;
}

// ---- by-products of the WTA scan (option "wta_outputs")
static int check_wta_outputs(srh_context *c, int slot, bool costs) {
	const ViewHost &v = c->views[slot];
	if (!(v.wta_flags & v.wta_asked)) return fail(SRH_E_INVALID, "view slot %d holds no WTA outputs (option \"wta_outputs\" off, no WTA pass since the upload, or its depth map came from the MRF stage)", slot);
	if (costs && !(v.wta_flags & v.wta_asked & SRH_WTA_COSTS)) return fail(SRH_E_INVALID, "view slot %d kept the winners only (wta_outputs = 1): no cost planes", slot);
	return SRH_OK;
}

extern "C" int srh_view_wta_outputs_state(srh_context *c, int slot, int *flags, int *oth_slot) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	const ViewHost &v = c->views[slot];
	if (flags) *flags = v.wta_flags & v.wta_asked;
	if (oth_slot) *oth_slot = (v.wta_flags & v.wta_asked) ? v.wta_oth : -1;
	return SRH_OK;
}

extern "C" int srh_view_wta_outputs_device(srh_context *c, int slot, void **win_xy, void **runner_xy, void **min_cost, void **second_cost) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if ((rc = check_wta_outputs(c, slot, min_cost || second_cost))) return rc;
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	if (win_xy) *win_xy = v.wta_xy;
	if (runner_xy) *runner_xy = v.wta_xy + 2*n;
	if (min_cost) *min_cost = v.wta_cost;
	if (second_cost) *second_cost = v.wta_cost + n;
	return SRH_OK;
}

extern "C" int srh_view_wta_outputs(srh_context *c, int slot, int32_t *win_xy, int32_t *runner_xy, double *min_cost, double *second_cost) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if ((rc = check_wta_outputs(c, slot, min_cost || second_cost))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	if (win_xy) HIP_TRY(hipMemcpyAsync(win_xy, v.wta_xy, 2*n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	if (runner_xy) HIP_TRY(hipMemcpyAsync(runner_xy, v.wta_xy + 2*n, 2*n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	if (min_cost) HIP_TRY(hipMemcpyAsync(min_cost, v.wta_cost, n*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (second_cost) HIP_TRY(hipMemcpyAsync(second_cost, v.wta_cost + n, n*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// ---- what option "subpixel" did to the pixels of the slot's last pass (srh_subpixel.hip)
static int check_subpixel(srh_context *c, int slot) {
	const ViewHost &v = c->views[slot];
	if (!v.wta_flags || !v.subpx) return fail(SRH_E_INVALID, "view slot %d holds no sub-pixel planes (option \"subpixel\" off, no WTA pass since the upload, or its depth map came from the MRF / SGM stage)", slot);
	return SRH_OK;
}

extern "C" int srh_view_subpixel_device(srh_context *c, int slot, void **delta, void **neigh_xy, void **cls) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if ((rc = check_subpixel(c, slot))) return rc;
	const ViewHost &v = c->views[slot];
	if (delta) *delta = v.subpx_delta;
	if (neigh_xy) *neigh_xy = v.subpx_neigh;
	if (cls) *cls = v.subpx_cls;
	return SRH_OK;
}

extern "C" int srh_view_subpixel(srh_context *c, int slot, double *delta, int32_t *neigh_xy, uint8_t *cls) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if ((rc = check_subpixel(c, slot))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	if (delta) HIP_TRY(hipMemcpyAsync(delta, v.subpx_delta, n*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (neigh_xy) HIP_TRY(hipMemcpyAsync(neigh_xy, v.subpx_neigh, 4*n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	if (cls) HIP_TRY(hipMemcpyAsync(cls, v.subpx_cls, n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// (the counts are taken from the planes when asked for: a pass pays nothing for them)
extern "C" int srh_view_subpixel_info(srh_context *c, int slot, srh_subpixel_info *info) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!info) return fail(SRH_E_INVALID, "null output");
	if ((rc = check_subpixel(c, slot))) return rc;
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	std::vector<uint8_t> k(n);
	std::vector<double> d(n);
	if ((rc = srh_view_subpixel(c, slot, d.data(), nullptr, k.data()))) return rc;
	memset(info, 0, sizeof(*info));
	for (size_t i = 0; i < n; ++i) {
		if (k[i] <= SRH_SUBPX_REFINED) ++info->n_class[k[i]];
		if (k[i] == SRH_SUBPX_REFINED && d[i] != 0) ++info->n_moved;
	}
	return SRH_OK;
}

extern "C" int srh_view_depth_copy_to_device(srh_context *c, int slot, void *dst_dev, size_t dst_bytes) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!dst_dev) return fail(SRH_E_INVALID, "null destination");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if (dst_bytes < (size_t)v.w*v.h*sizeof(double))
		return fail(SRH_E_INVALID, "destination of %zu bytes is smaller than the %dx%d depth map of slot %d", dst_bytes, v.w, v.h, slot);
	HIP_TRY(hipMemcpyAsync(dst_dev, v.depth, (size_t)v.w*v.h*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
	return SRH_OK;
}

extern "C" int srh_view_depth_copy_from_device(srh_context *c, int slot, const void *src_dev, size_t src_bytes) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!src_dev) return fail(SRH_E_INVALID, "null source");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if (src_bytes < (size_t)v.w*v.h*sizeof(double))
		return fail(SRH_E_INVALID, "source of %zu bytes is smaller than the %dx%d depth map of slot %d", src_bytes, v.w, v.h, slot);
	HIP_TRY(hipMemcpyAsync(v.depth, src_dev, (size_t)v.w*v.h*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
	return SRH_OK;
}

// ------------------------------------------------------------------ runs
// bytes of device memory the band buffers hold now (they are re-used or re-allocated by the next run)
static size_t held_band_bytes(srh_context *c) {
	size_t b = 0;
	c->each_scratch([&](Scratch &m) { b += m.band.bytes(); });
	for (const ViewHost &v : c->views) b += v.geo5.bytes();                 // (released with the band buffers)
	return b;
}

// The band budget of a run: what the caller asked for, but no more than a quarter of what the device can give right now
// (free memory + what the band buffers already hold): the MultiViewStereo path treats the budget as a target (bands up
// to 1.25x) and keeps two views' band buffers, the TwoView path adds the per-pixel constant planes.  A GPU shared with
// other processes, several contexts on one GPU or a smaller device get thinner bands instead of an allocation failure.
static size_t band_budget(srh_context *c) {
	size_t b = c->wbuf_budget;
	if (c->budget_cap && b > c->budget_cap) b = c->budget_cap;
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
		size_t avail = free_b + held_band_bytes(c) + pool_bytes_on(c->device);   // (the pool's blocks are this context's to take)
		if (c->mem_limit && avail > c->mem_limit) avail = c->mem_limit;
		if (b > avail/4) b = avail/4;
	} else (void)hipGetLastError();
	if (b < ((size_t)1 << 20)) b = (size_t)1 << 20;
	c->budget_used = b;
	return b;
}

static void release_band_buffers(srh_context *c) {
	pool_flush(c->device);                                        // (out of memory: the pool's blocks go back to the driver first)
	c->each_scratch([](Scratch &m) { m.band.free(); });           // (called with every stream of the context drained)
	// the geodesic_dma_kernel's second copy of the edge / tap planes (42 B per pixel and view, made on first use): memory an
	// out-of-memory retry must be able to reclaim -- the register-staged kernel needs no such copy and serves the view until
	// it is uploaded again
	for (ViewHost &v : c->views)
		if (v.geo5) { v.geo5.free(); v.geo5_valid = false; v.geo5_denied = true; }
}

// Run `body`; when it fails because a band buffer could not be allocated, wait for everything in flight, release the
// band buffers, halve the band budget and run it again -- down to one-megabyte bands (a band is at least one image row).
template <class F>
static int with_thinner_bands(srh_context *c, F body) {
	for (;;) {
		g_oom = false;
		g_alloc_limit = c->alloc_limit;
		const int rc = body();
		if (rc != SRH_E_DEVICE || !g_oom) return rc;
		g_oom = false;
		const size_t used = c->budget_used;
		if (used <= ((size_t)1 << 20)) return rc;                   // already the thinnest bands there are
		// Everything in flight is drained before the band buffers go.  A MultiViewStereo view queued earlier on the other
		// slot stays PENDING: its kernels are complete now, but its list-capacity check (mvs_settle_slot: h_maxc is pinned
		// and stays valid) has not been made -- the retried call, or whichever entry point comes next, settles it and
		// redoes the view if a list was cut.
		c->wait_streams();                                          // (either TwoView pass's, the slots', the side stream)
		release_band_buffers(c);
		c->budget_cap = used/2;
		c->stats.band_retries += 1;
	}
}

static int band_rows(srh_context *c, int W, int H, int T) {
	size_t rows = band_budget(c) / ((size_t)T*sizeof(double)*(size_t)W);
	if (rows < 1) rows = 1;
	if (rows > (size_t)H) rows = H;
	return (int)rows;
}

// `bytes` of device memory to the host, behind everything queued on `st`, and the wait for them
static int read_back(hipStream_t st, void *host, const void *dev, size_t bytes) {
	HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return SRH_OK;
}

static int fetch_counters(srh_context *c, const Lane &lane, int used_dense) {
	Counters h;
	int rc;
	if ((rc = read_back(lane.stream, &h, lane.mem->cnt, sizeof(h)))) return rc;
	c->stats.n_pixels = (int64_t)h.n_pixels;
	c->stats.n_eval = (int64_t)h.n_eval;
	c->stats.n_eval_device = (int64_t)h.n_eval_device;
	c->stats.scan_tiles_template = (int64_t)h.scan_tiles_template;
	c->stats.scan_tiles_walked = (int64_t)h.scan_tiles_walked;
	c->stats.scan_tiles_bound = (int64_t)h.scan_tiles_bound;
	c->stats.mvs_waves_staged = (int64_t)h.mvs_waves_staged;
	c->stats.mvs_waves_listed = (int64_t)h.mvs_waves_listed;
	c->stats.used_dense_path = used_dense;
	c->stats.used_fused_kernel = c->last_fused ? 1 : 0;
#ifdef SRH_PROFILE_PHASES
	{
		unsigned long long g[8];
		geodesic_phases_fetch(g);
		if (g[7])
			fprintf(stderr, "[srh prof] geodesic kernel: %llu waves, cycles per wave: staging %.0f  sweeps %.0f  exp %.0f  rows out %.0f  pconst: first sweep %.0f  second sweep %.0f  rest %.0f\n",
			        g[7], (double)g[0]/g[7], (double)g[1]/g[7], (double)g[2]/g[7], (double)g[4]/g[7], (double)g[5]/g[7], (double)g[6]/g[7], (double)g[3]/g[7]);
	}
	if (h.dbg_redo[4])
		fprintf(stderr, "[srh prof] redo kernel: %llu pixels, cycles per pixel (first wave): projections + mask %.0f  walk %.0f  wait for the columns %.0f  "
		        "running minimum %.0f | second wave: columns %.0f\n", h.dbg_redo[4], (double)h.dbg_redo[0]/h.dbg_redo[4], (double)h.dbg_redo[1]/h.dbg_redo[4],
		        (double)h.dbg_redo[2]/h.dbg_redo[4], (double)h.dbg_redo[3]/h.dbg_redo[4], (double)h.dbg_redo[5]/h.dbg_redo[4]);
	if (h.dbg_waves && h.dbg_blocks && h.dbg_phase[3] && h.strip_ticket) {
		const double nw = (double)h.dbg_waves, nt = (double)h.dbg_blocks/nw;
		fprintf(stderr, "[srh dbg] strip: waves %llu, tiles/wave %.1f (%.1f with phase 2), cycles/wave %.0f | per tile: ticket %.0f  own requests %.0f  barriers %.0f  setup %.0f  "
		        "block loops %.0f  p2 lists %.0f  p2 blocks %.0f  p2 singles %.0f\n", h.dbg_waves, nt, (double)h.dbg_cycles/nw, (double)h.dbg_total_cycles/nw,
		        h.dbg_phase[0]/nw/nt, h.dbg_phase[1]/nw/nt, h.dbg_phase[2]/nw/nt, h.dbg_phase[3]/nw/nt, h.dbg_phase[4]/nw/nt,
		        h.dbg_phase[5]/nw/nt, h.dbg_phase[6]/nw/nt, h.dbg_phase[7]/nw/nt);
		static const char *names[8] = { "ticket", "own requests", "barriers", "setup", "block loops", "p2 lists", "p2 blocks", "p2 singles" };
		const int nwv = h.dbg_wave[8*4 + 4] ? 8 : 4;
		for (int k = 0; k < 8; ++k) {
			fprintf(stderr, "[srh dbg]   %-13s by wave:", names[k]);
			for (int w = 0; w < nwv; ++w) fprintf(stderr, " %8.0f", h.dbg_wave[8*k + w]/((double)h.dbg_blocks/nwv));
			fprintf(stderr, "\n");
		}
	} else
	if (h.dbg_waves && !c->last_fused)
		fprintf(stderr, "[srh dbg] dense: waves %llu, cycles/wave %.0f, fast blocks/wave %.1f, cycles/fast block %.0f\n",
		        h.dbg_waves, (double)h.dbg_total_cycles/h.dbg_waves, (double)h.dbg_blocks/h.dbg_waves,
		        h.dbg_blocks ? (double)h.dbg_cycles/h.dbg_blocks : 0.0);
	if (h.dbg_waves && !c->last_fused && !h.strip_ticket)
		fprintf(stderr, "[srh dbg] phases/wave: stage_w %.0f prologue %.0f sync %.0f stage_rt %.0f compute %.0f tail %.0f\n",
		        (double)h.dbg_phase[0]/h.dbg_waves, (double)h.dbg_phase[1]/h.dbg_waves, (double)h.dbg_phase[2]/h.dbg_waves,
		        (double)h.dbg_phase[3]/h.dbg_waves, (double)h.dbg_phase[4]/h.dbg_waves, (double)h.dbg_phase[5]/h.dbg_waves);
	if (h.dbg_waves && c->last_fused)
		fprintf(stderr, "[srh dbg] fused: %llu tiles, %llu with select-form work, %llu pixels with an unusable tap of their own\n",
		        h.dbg_waves, h.n_listed, h.n_slots);
	if (h.dbg_waves && c->last_fused)
		fprintf(stderr, "[srh dbg] fused, role wave cycles/tile: A geometry %.0f  B accept %.0f  C stage %.0f  D prologue %.0f  E1 blocks %.0f  E2 general %.0f  F wta %.0f  barriers %.0f | other waves: blocks %.0f barriers %.0f total %.0f\n",
		        (double)h.dbg_phase[0]/h.dbg_waves, (double)h.dbg_phase[1]/h.dbg_waves, (double)h.dbg_phase[2]/h.dbg_waves,
		        (double)h.dbg_phase[3]/h.dbg_waves, (double)h.dbg_phase[4]/h.dbg_waves, (double)h.dbg_phase[5]/h.dbg_waves,
		        (double)h.dbg_phase[6]/h.dbg_waves, (double)h.dbg_phase[7]/h.dbg_waves,
		        (double)h.dbg_cycles/(3.0*h.dbg_waves), (double)h.dbg_blocks/(3.0*h.dbg_waves), (double)h.dbg_total_cycles/(3.0*h.dbg_waves));
	if (h.dbg_phase[6] && !c->last_fused)
		fprintf(stderr, "[srh dbg] rows: tasks %llu fast %llu, rows/pixel %.2f, slots/px %.1f, wave iterations %llu all-fast %llu\n",
		        h.dbg_phase[6], h.dbg_phase[7], (double)h.dbg_cycles/(double)h.n_pixels, 8.0*h.dbg_phase[6]/(double)h.n_pixels,
		        h.dbg_blocks, h.dbg_total_cycles);
	if (h.dbg_phase[6] && !c->last_fused && h.dbg_wave[8])
		fprintf(stderr, "[srh dbg] rows cost kernel, wave tiles %llu: cycles per tile: staging %.0f  constants %.0f  phase 1 %.0f  p2 blocks %.0f  p2 singles %.0f | tiles with blocks %llu (%llu blocks: %.0f cycles per such tile), with singles %llu (%llu singles: %.0f cycles per such tile); rounds if the tile's tasks were dealt to its 64 lanes: %.2f per tile\n",
		        h.dbg_wave[8], (double)h.dbg_wave[0]/h.dbg_wave[8], (double)h.dbg_wave[1]/h.dbg_wave[8], (double)h.dbg_wave[2]/h.dbg_wave[8],
		        (double)h.dbg_wave[3]/h.dbg_wave[8], (double)h.dbg_wave[4]/h.dbg_wave[8], h.dbg_wave[9], h.dbg_wave[10],
		        h.dbg_wave[9] ? (double)h.dbg_wave[3]/h.dbg_wave[9] : 0.0, h.dbg_wave[11], h.dbg_wave[12], h.dbg_wave[11] ? (double)h.dbg_wave[4]/h.dbg_wave[11] : 0.0, (double)h.dbg_wave[13]/h.dbg_wave[8]);
#endif
	return SRH_OK;
}

// support windows of rows [by, by+nr) of view `ref` into the lane's wbuf
static void run_weights(srh_context *c, const Lane &lane, int ref, int W, const srh_params &p, int by, int nr, size_t wstride,
                        double *pconst = nullptr, bool wimg = false) {
	if (p.weight_kind == SRH_WEIGHT_GEODESIC && !c->force_generic && wimg && c->geodma && p.window_radius == 5 && !c->views[ref].geo5_denied) {
		// the dense path's windows: tiles by LDS-DMA from planes with their borders written out (made once per uploaded view)
		ViewHost &v = c->views[ref];
		bool ok = true;
		if (!v.geo5) {
			if (v.geo5.alloc(geo5_doubles(v.w, v.h)) != hipSuccess) ok = false;   // (no room: the register-staged kernel needs no second copy)
			v.geo5_valid = false;
		}
		if (ok && !v.geo5_valid) {
			Scope s(c, lane.stream, "geo5_planes_kernel");
			launch_geo5_planes(lane.stream, v.edges, v.gray_tv, v.mask, v.w, v.h, v.geo5);
			v.geo5_valid = true;
		}
		if (ok) {
			Scope s(c, lane.stream, "geodesic_dma_kernel");
			if (launch_geodesic_dma(lane.stream, c->d_views, ref, W, v.geo5, p, by, nr, lane.mem->band.wbuf, pconst, c->num_cus)) return;
		}
	}
	if (p.weight_kind == SRH_WEIGHT_GEODESIC && !c->force_generic) {
		Scope s(c, lane.stream, "geodesic_reg_kernel");
		if (launch_geodesic_reg(lane.stream, c->d_views, ref, W, c->views[ref].edges, p, by, nr, lane.mem->band.wbuf, wstride, pconst, wimg)) return;
	}
	if (p.weight_kind == SRH_WEIGHT_ADAPTIVE && !c->force_generic) {
		Scope s(c, lane.stream, "adaptive_reg_kernel");
		if (launch_adaptive_reg(lane.stream, c->d_views, ref, W, p, by, nr, lane.mem->band.wbuf, wstride, pconst, wimg)) return;
	}
	Scope s(c, lane.stream, "weights_kernel");
	launch_weights(lane.stream, c->d_views, ref, W, p, by, nr, lane.mem->band.wbuf, wstride, pconst, wimg);
}

// (the rig test that proposes the dense path, rig_is_row_aligned: srh_rectify.hpp)

// The WTA by-products of a pass ref -> oth (option "wta_outputs"): the planes exist and hold either what an earlier pass of
// the same kind left (a pass over some rows writes those rows only, as it does in the depth map) or the "none" values.
// Allocated like the view's other planes; a refusal is a clean SRH_E_DEVICE before the pass queues anything.  Option off:
// no allocation, no launch -- the slot's planes, if any, no longer describe its depth map.
static int ensure_wta_planes(srh_context *c, hipStream_t st, int ref, int oth) {
	ViewHost &v = c->views[ref];
	const int keep = c->wta_keep();
	if (!keep) { v.wta_flags = 0; v.subpx = false; return SRH_OK; }
	const size_t n = (size_t)v.w*v.h;
	const bool subpx = c->subpixel != 0;
	v.wta_asked = c->wta_outputs;
	if (v.wta_flags == keep && v.wta_oth == oth && v.subpx == subpx) return SRH_OK;
	if (!v.wta_xy) HIP_TRY(v.wta_xy.alloc(4*n));
	if ((keep & SRH_WTA_COSTS) && !v.wta_cost) HIP_TRY(v.wta_cost.alloc(2*n));
	if (subpx) {
		if (!v.subpx_delta) HIP_TRY(v.subpx_delta.alloc(n));
		if (!v.subpx_neigh) HIP_TRY(v.subpx_neigh.alloc(4*n));
		if (!v.subpx_cls) HIP_TRY(v.subpx_cls.alloc(n));
	}
	HIP_TRY(hipMemsetAsync(v.wta_xy, 0xff, 4*n*sizeof(int32_t), st));           // (-1, -1): no winner, no runner-up
	if (keep & SRH_WTA_COSTS) launch_fill(st, v.wta_cost, 2*n, __builtin_inf());
	if (subpx) {                                                                 // no pixel refined, no neighbour, class NONE
		HIP_TRY(hipMemsetAsync(v.subpx_delta, 0, n*sizeof(double), st));
		HIP_TRY(hipMemsetAsync(v.subpx_neigh, 0xff, 4*n*sizeof(int32_t), st));
		HIP_TRY(hipMemsetAsync(v.subpx_cls, SRH_SUBPX_NONE, n, st));
	}
	v.wta_flags = keep; v.wta_oth = oth; v.subpx = subpx;
	return SRH_OK;
}

// A first guess of a pair's list capacities, before any pass has measured them (the list path of srh_twoview_wta):
// cmax = candidates per pixel, smax = cost slots per pixel (row runs in 8-column blocks).  A curve's candidates are the
// raster points of its kept segments with the joints counted once, so at most the Chebyshev length of the polyline through
// the kept label points + 1, and its slots at most that + 8 per image row it touches.  The host walks a coarse polyline
// (nine labels) for a grid of reference pixels with the very camera model the kernels use (srh_geom.hpp), takes the longest,
// and adds a margin for what nine labels do not see.  Too small a guess repeats the pass with the measured maximum.
static void estimate_list_capacity(const srh_camera &rc, const srh_camera &oc, int W, int H, int OW, int OH,
                                   const srh_params &p, int y0, int y1, int &cmax, int &smax, bool mvs = false)
{
	(void)H;
	const int D = p.num_depth_levels, NL = D < 9 ? D : 9, GX = 13, GY = 9;   // (the grid includes the band's border rows and columns:
	                                                                          // distortion and refraction stretch the curves most there)
	const Vec3 normal = load3(rc.pdir);
	long best_len = 0, best_rows = 0;
	for (int gy = 0; gy < GY; ++gy)
		for (int gx = 0; gx < GX; ++gx) {
			const int x = (int)((gx*(long)(W - 1))/(GX - 1)), y = y0 + (int)((gy*(long)(y1 - y0 - 1))/(GY - 1));
			const Ray ray = cam_unproject(rc, (x + 0.5)/p.image_scale, (y + 0.5)/p.image_scale);
			long len = 0, rows = 0;
			bool have = false;
			int px = 0, py = 0;
			for (int k = 0; k < NL; ++k) {
				const int d = NL > 1 ? (int)(((long)k*(D - 1))/(NL - 1)) : 0;
				Vec3 point = load3(rc.C);                          // (in: the camera centre, out: the label's point on the ray)
				if (!point_from_depth(ray, normal, depth_from_label(p, mvs, d), point)) continue;
				if (!cam_project(oc, point)) continue;
				// (clamped a little outside the other image: what lies further out is no candidate)
				const double cxd = fmin(fmax(point.x*p.image_scale, -64.0), (double)OW + 64.0);
				const double cyd = fmin(fmax(point.y*p.image_scale, -64.0), (double)OH + 64.0);
				if (!(cxd == cxd) || !(cyd == cyd)) continue;
				const int ix = (int)cxd, iy = (int)cyd;
				if (have) {
					const long dx = labs((long)ix - px), dy = labs((long)iy - py);
					len += dx > dy ? dx : dy;
					rows += dy;
				}
				have = true; px = ix; py = iy;
			}
			if (len > best_len) best_len = len;
			if (rows > best_rows) best_rows = rows;
		}
	if (best_rows > SRH_ROWS_NR) best_rows = SRH_ROWS_NR;
	// + 12 % for what nine labels do not see, + one entry per kept segment: a list holds a segment's both end points, the
	// joint of two segments twice (the C5 rig's corner pixel: 379 distinct candidates, 157 joints, a list of 536)
	// (MultiViewStereo's lists drop consecutive duplicates, std::unique: no joint term there)
	long cm = best_len + best_len/8 + (mvs ? 0 : (best_len < D - 1 ? best_len : D - 1)) + 40;
	if (cm > 65520) cm = 65520;
	cmax = (int)((cm + 7) & ~7L);
	long sm = cmax + 8*(best_rows + 2) + 32;
	if (sm > 65528) sm = 65528;
	smax = (int)((sm + 7) & ~7L);
}

// The NaN-bordered gray_tv plane of a view (the strip kernels' taps; the general cost of the left-out columns and of the
// certified redo reads it without bound tests), made on first use after an upload, on `st`
static int ensure_tvp(srh_context *c, hipStream_t st, ViewHost &v) {
	if (!v.tvp) HIP_TRY(v.tvp.alloc(padded_size(v.w, v.h)));
	if (!v.tvp_valid) {
		Scope s(c, st, "padded_plane_kernel");
		launch_padded_plane(st, v.gray_tv, v.w, v.h, v.tvp);
		v.tvp_valid = true;
	}
	return SRH_OK;
}

// cost_sad's "window fully usable" plane of radius R (its zero-bordered copy, if any, is stale then)
static int ensure_fulls(srh_context *c, hipStream_t st, ViewHost &v, int R) {
	if (v.fulls_r == R) return SRH_OK;
	if (!v.fulls) HIP_TRY(v.fulls.alloc((size_t)v.w*v.h));
	Scope s(c, st, "sad_full_window_kernel");
	launch_sad_full_window(st, v.mask, v.w, v.h, R, v.fulls);
	v.fulls_r = R;
	v.fullsp_r = 0;
	return SRH_OK;
}

// The census signatures of a view (option "cost" = SRH_COST_CENSUS), made on first use after an upload, on `st`; the
// kernels find the plane through the slot's ViewDev
static int ensure_census(srh_context *c, hipStream_t st, int slot) {
	ViewHost &v = c->views[slot];
	if (v.census_valid) return SRH_OK;
	if (!v.census) {
		HIP_TRY(v.census.alloc((size_t)v.w*v.h));
		const uint64_t *dp = v.census;
		HIP_TRY(hipMemcpyAsync((char *)(ViewDev *)(c->d_views + slot) + offsetof(ViewDev, census), &dp, sizeof(dp), hipMemcpyHostToDevice, st));
		HIP_TRY(hipStreamSynchronize(st));                          // (`dp` goes away)
	}
	Scope s(c, st, "census_kernel");
	launch_census(st, v.gray, v.w, v.h, v.census);
	v.census_valid = true;
	v.cenp_valid = false;
	return SRH_OK;
}

// cost_ncc's "window fully usable" plane of radius R, with its two counts behind it (option "rows_masked")
static int ensure_full(srh_context *c, hipStream_t st, ViewHost &v, int R) {
	if (v.full_r == R) return SRH_OK;
	Scope s(c, st, "full_window_kernel");
	uint32_t *stat = (uint32_t *)(v.full + full_stat_offset((size_t)v.w*v.h));
	HIP_TRY(hipMemsetAsync(stat, 0, 2*sizeof(uint32_t), st));
	launch_full_window(st, v.gray_tv, v.w, v.h, R, v.full, stat);
	v.full_r = R;
	return SRH_OK;
}

// the zero-bordered copy of cost_sad's "window fully usable" plane of radius R (the SAD and the census strip kernels')
static int ensure_fullsp(srh_context *c, hipStream_t st, ViewHost &v, int R) {
	int rc;
	if ((rc = ensure_fulls(c, st, v, R))) return rc;
	if (!v.fullsp) HIP_TRY(v.fullsp.alloc(padded_size(v.w, v.h)));
	if (v.fullsp_r != R) {
		Scope s(c, st, "padded_bytes_kernel");
		launch_padded_bytes(st, v.fulls, v.w, v.h, v.fullsp);
		v.fullsp_r = R;
	}
	return SRH_OK;
}

// The planes twoview_strip_sad_kernel stages from (option "sad_dense"), made on first use after an upload, on `st`:
// the NaN-bordered gray_tv plane (the reference side's taps), the NaN-bordered masked gray plane (the other side's) and the
// zero-bordered copy of cost_sad's "window fully usable" plane of radius R
static int ensure_sad_planes(srh_context *c, hipStream_t st, ViewHost &v, int R) {
	int rc;
	if ((rc = ensure_tvp(c, st, v))) return rc;
	if (!v.grayp) HIP_TRY(v.grayp.alloc(padded_size(v.w, v.h)));
	if (!v.grayp_valid) {
		Scope s(c, st, "padded_gray_kernel");
		launch_padded_gray(st, v.gray, v.mask, v.w, v.h, v.grayp);
		v.grayp_valid = true;
	}
	return ensure_fullsp(c, st, v, R);
}

// The planes twoview_strip_census_kernel stages from (option "census_dense"), made on first use after an upload, on `st`:
// the view's signatures on the padded raster, once as the other side's taps and once as the reference side's, and the
// zero-bordered copy of cost_sad's "window fully usable" plane of radius R (the same definition of "fully usable")
static int ensure_census_planes(srh_context *c, hipStream_t st, int slot, int R) {
	ViewHost &v = c->views[slot];
	int rc;
	if ((rc = ensure_census(c, st, slot))) return rc;
	if (!v.cenothp) HIP_TRY(v.cenothp.alloc(padded_size(v.w, v.h)));
	if (!v.cenrefp) HIP_TRY(v.cenrefp.alloc(padded_size(v.w, v.h)));
	if (!v.cenp_valid) {
		Scope s(c, st, "padded_census_kernel");
		launch_padded_census(st, v.census, v.mask, v.gray_tv, v.w, v.h, v.cenothp, v.cenrefp);
		v.cenp_valid = true;
	}
	return ensure_fullsp(c, st, v, R);
}

// ---- the TwoView WTA pass driver: a pass descriptor, a plan that launches nothing, one runner per path (fused kernel,
// candidate lists, dense plan, walk kernel) and a controller that reads their outcomes (twoview_wta_run) ----------------

// dense: the row-aligned kernels are *proposed* (the scan kernel verifies every candidate), cost rows of cstride doubles;
// fused: the candidate range fits an LDS cost row of srh_fused.hip
struct TvPlan { bool dense = false; int cstride = 0; bool fused = false; };
// The candidate lists of a pass: capacities cmax = candidates, smax = cost slots (row runs in 8-column blocks) per pixel;
// guessed: they are the host's first guess; rows_mode: row runs (srh_rows.hip), else list order (srh_list.hip); cert: row
// runs in the certified arithmetic; lrows: rows per band
struct TvLists { int cmax = 0, smax = 0; bool rows_mode = false, guessed = false, cert = false; size_t lrows = 0; };
// An attempt of the dense plan: the plan's cstride; strip: the persistent strip form of the cost kernel, the band's windows
// in the LDS image's layout then; cert: certified arithmetic (fused cost loops + the certified scan and redo); rows per band
// tables_pending: label table and scan template are still to be queued, on the side stream beside the first band's windows;
// tpl_wait: the template is queued there and the pass's stream has not waited for it yet (the first scan does)
struct TvDense { int cstride = 0; bool strip = false, cert = false, tscan = false; size_t rows = 0; int lanes = 8;
                 bool tables_pending = false, tpl_wait = false; };

// One pass ref -> oth over rows [y0, y1) of equal-sized views (clamped to the view: y1 <= y0, nothing to do): what every
// runner needs.  lane: the stream the pass is queued on and the scratch it writes; R, T: window radius and taps; budget:
// bytes of band scratch.
// wout, the by-products of the scan (option "wta_outputs"): every scan kernel of the pass stores winner and runner-up where
// it stores the depth, and twoview_winner_costs_kernel follows the band's last scan with their exact costs.  A repeated
// attempt rewrites every row of the pass, so the planes hold what the attempt whose depth map stands wrote.
struct TvPass {
	srh_context *c = nullptr;
	Lane lane = { nullptr, nullptr };
	int ref = 0, oth = 0;
	const srh_params *p = nullptr;
	int W = 0, H = 0, y0 = 0, y1 = 0, R = 0, T = 0;
	size_t budget = 0;
	int kind = SRH_COST_NCC;                  // option "cost"; sad / census: the kind is SRH_COST_SAD / SRH_COST_CENSUS
	bool sad = false, census = false;
	bool strip_only = false;                  // cost_sad and the census cost: on the dense plan the strip form only, every column written
	int32_t *wout = nullptr;
	const double *subpx_tdist = nullptr;      // option "subpixel": the pass's label plane table (label_plane_table_kernel)

	size_t rows_per_band(size_t bytes) const;
	void winner_costs(int by, int nr, bool wimg_layout) const;
	TvPlan plan() const;
	int run_fused(bool &stands) const;
	int lists_prepare(TvLists &S) const;
	int lists_rows_band(const TvLists &S, int by, int nr) const;
	int lists_pass(TvLists &S) const;
	int run_lists(bool cert_ok, srh_context::TvDefer *defer) const;
	int dense_prepare(TvDense &D) const;
	void dense_tables(const Lane &on, const TvDense &D, bool table, bool tpl) const;
	bool dense_fill_padded(const TvDense &D, int arith) const;
	int dense_band_inputs(TvDense &D, int by, int nr, int arith) const;
	int dense_cost_pass(const TvDense &D, int by, int nr, int arith, bool raw) const;
	int run_dense(TvDense &D) const;
	int run_walk() const;
};

static int tv_pass_init(TvPass &P, srh_context *c, const Lane &lane, int ref, int oth, const srh_params *p, int y0, int y1) {
	if (ref == oth) return fail(SRH_E_INVALID, "ref and other view are the same slot");
	const ViewHost &L = c->views[ref], &Rv = c->views[oth];
	if (L.w != Rv.w || L.h != Rv.h)
		return fail(SRH_E_INVALID, "TwoViewStereo needs equal-sized views (%dx%d vs %dx%d; twoviewstereo.cpp:116-119)",
		            L.w, L.h, Rv.w, Rv.h);
	HIP_TRY(hipSetDevice(c->device));
	P.c = c; P.lane = lane; P.ref = ref; P.oth = oth; P.p = p;
	P.W = L.w; P.H = L.h;
	P.y0 = y0 < 0 ? 0 : y0;
	P.y1 = (y1 <= 0 || y1 > P.H) ? P.H : y1;
	P.R = p->window_radius;
	P.T = (2*P.R + 1)*(2*P.R + 1);
	P.kind = c->cost_kind;
	P.sad = P.kind == SRH_COST_SAD;
	P.census = P.kind == SRH_COST_CENSUS;
	P.strip_only = P.sad || P.census;
	if (P.y1 > P.y0) P.budget = band_budget(c);
	return SRH_OK;
}

// rows per band: what the budget holds at `bytes` per pixel, at least one, at most the pass
size_t TvPass::rows_per_band(size_t bytes) const {
	return std::min(std::max<size_t>(budget/(bytes*(size_t)W), 1), (size_t)(y1 - y0));
}

void TvPass::winner_costs(int by, int nr, bool wimg_layout) const {
	if (!wout || !(c->wta_keep() & SRH_WTA_COSTS)) return;
	const ViewHost &v = c->views[ref];
	double *mc = v.wta_cost;
	{ Scope s(c, lane.stream, "twoview_winner_costs_kernel");
	  launch_twoview_winner_costs(lane.stream, c->d_views, ref, oth, W, *p, kind, by, nr, lane.mem->band.wbuf, wimg_layout,
	                              wout, mc, mc + (size_t)W*H); }
	if (!c->subpixel) return;
	// option "subpixel": the band's winners, their costs and its depths are final here and its windows still in the buffer.
	// A repeated attempt rewrites the rows' depths and winners first and is refined again: the planes follow the attempt that stands.
	{ Scope s(c, lane.stream, "subpixel_neighbours_kernel");
	  launch_subpixel_neighbours(lane.stream, c->d_views, ref, oth, W, *p, by, nr, subpx_tdist, wout, v.subpx_neigh, v.subpx_cls); }
	{ Scope s(c, lane.stream, "subpixel_refine_kernel");
	  launch_subpixel_refine(lane.stream, c->d_views, ref, oth, W, *p, kind, by, nr, lane.mem->band.wbuf, wimg_layout, wout, mc,
	                         v.subpx_neigh, v.subpx_cls, v.subpx_delta); }
}

// The exact redo of flagged pixels is launched for a CAPACITY -- the whole band: the list buffer holds every pixel of it,
// the redo kernels share the list in grid-stride loops and read the count on the device -- so however many pixels flag
// (adversarial images: exact ties everywhere) each is redone once, the host never waits for the count, and no pass is
// ever repeated as a whole for it.  (Round 4 launched for 1/32 of the band, at most 16 384 pixels, and repeated the
// whole pass in mode 0 beyond that: a cliff at 0.79 % of C3.)
static int redo_capacity(size_t band_pixels) { return (int)std::min<size_t>(band_pixels, (size_t)1 << 30); }

// widest candidate range a pixel of a row-aligned rig can have, in columns: disparity(min_depth) - disparity(max_depth)
static double disparity_span(const srh_params &p, double fx_bx) {
	return fx_bx*p.image_scale*fabs(1.0/p.min_depth - 1.0/p.max_depth);
}

// ---- plan: dense row-aligned kernels (or the fused kernel), or the general kernels.  Launches nothing.
// (cost_sad: the dense plan only with option "sad_dense", its cost rows filled by twoview_strip_sad_kernel; no per-tile
// and no fused kernel -- without the option rectified rigs take the row-run lists too; DESIGN.md 4c.  The census cost
// likewise: option "census_dense", twoview_strip_census_kernel)
TvPlan TvPass::plan() const {
	const ViewHost &L = c->views[ref], &Rv = c->views[oth];
	TvPlan pl;
	pl.dense = !c->force_generic && (!census || c->census_dense) && (!sad || c->sad_dense) && (R == 5 || R == 2);
	double fx_bx = 0;
	if (pl.dense && !rig_is_row_aligned(L.cam, Rv.cam, &fx_bx)) {
		// test hook: any pinhole pair may be *proposed* (the scan kernel refutes the proposal, see the controller's redo)
		const bool pinhole = !L.cam.is_distorted && !Rv.cam.is_distorted && !L.cam.is_refractive && !Rv.cam.is_refractive;
		if (c->force_dense && pinhole) fx_bx = (double)(W + 8)/disparity_span(*p, 1.0);
		else pl.dense = false;
	}
	if (!pl.dense) return pl;
	const double span = disparity_span(*p, fx_bx);                // (+ margins: the stride)
	if (!(p->min_depth > 0) || !(p->max_depth > 0) || !(span < 4096.0)) pl.dense = false;
	else pl.cstride = (((int)ceil(span) + 3) + 7) & ~7;
	if (pl.cstride > W + 8) pl.cstride = (W + 8 + 7) & ~7;
	// cost_sad and the census cost have the strip form only: a range wider than its chunk takes the candidate lists
	if (strip_only && pl.dense && pl.cstride + SRH_WTILE > strip_chunk_columns()) pl.dense = false;
	pl.fused = pl.dense && !strip_only && c->use_fused && (c->arith == 0 || c->arith == 3) &&
	           p->num_depth_levels <= SRH_FUSED_MAXC && span + 1.0 <= (double)SRH_FUSED_MAXC;
	return pl;
}

// ---- row-aligned rig whose candidate range fits an LDS cost row: one fused kernel per band (srh_fused.hip).
// stands: the kernel had an instantiation and every curve was monotone, on its row and inside the LDS tile
int TvPass::run_fused(bool &stands) const {
	int rc;
	stands = false;
	HIP_TRY(hipMemsetAsync(lane.mem->cnt, 0, sizeof(Counters), lane.stream));
	if ((rc = lane.mem->band.tnum.ensure((size_t)p->num_depth_levels))) return rc;
	{ Scope s(c, lane.stream, "pinhole_label_table_kernel");
	  launch_pinhole_label_table(lane.stream, c->d_views, ref, *p, false, lane.mem->band.tnum); }
	const int rows = (int)rows_per_band((size_t)T*sizeof(double));
	if ((rc = lane.mem->band.wbuf.ensure(wbuf_doubles(W, rows, T)))) return rc;
	bool launched = true;
	for (int by = y0; by < y1 && launched; by += rows) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		const int nr = std::min(rows, y1 - by);
		run_weights(c, lane, ref, W, *p, by, nr, SRH_WTILE);
		Scope s(c, lane.stream, "twoview_fused_kernel");
		launched = launch_twoview_fused(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, lane.mem->band.tnum, lane.mem->cnt, wout);
		if (launched) winner_costs(by, nr, false);
	}
	HIP_TRY(hipGetLastError());
	if (!launched) return SRH_OK;
	Counters hc;
	if ((rc = read_back(lane.stream, &hc, lane.mem->cnt, sizeof(hc)))) return rc;
	stands = hc.not_row_aligned == 0;
	return SRH_OK;
}

// ---- arbitrary geometry: candidate lists, evaluated in row runs (srh_rows.hip) or in list order (srh_list.hip)

// every list and every pixel's cost slots fitted the capacities, no curve crossed more than SRH_ROWS_NR rows
// (mx: the kernels' maxima in the lane's span -- longest list, most cost slots, a curve over too many rows)
static bool tv_lists_fit(const int *mx, int cmax, int smax) {
	return mx[0] <= cmax && ((mx[1] + 7) & ~7) <= smax && mx[2] == 0;
}

// A standing row-run pass teaches the context its capacities, what later runs of the pair are queued with: the
// capacities the pass stood on -- or, when they were a guess, what the pass measured (the tight strides a counting pass
// would have given) -- and how the pair's lists are best evaluated: short spans (steep curves) fill their 8-column blocks
// badly, a slot costs ~0.4 of a candidate evaluated in list order, so beyond 2.2 slots per candidate the other path wins
static void tv_learn_lists(srh_context *c, int ref, int oth, bool guessed, int cmax, int smax, const int *mx, const Counters &h) {
	const int cm = guessed ? std::max(8, (mx[0] + 7) & ~7) : cmax;
	const int sm = guessed ? std::max(cm + 64, (mx[1] + 7) & ~7) : smax;
	if (cm > c->list_cmax_hint) c->list_cmax_hint = cm;
	if (sm > c->list_smax_hint) c->list_smax_hint = sm;
	c->views[ref].list_mode[oth] = (h.n_slots > 2.2*(double)h.n_listed) ? 2 : 1;
}

// srh_twoview_compute's optimistic passes: the counters (lists: and the kernels' maxima) travel to pinned memory behind
// the kernels, and the record says what the pass stood on; the caller verifies both passes with one wait (tv_pass_stands)
static int tv_defer_queue(const Lane &lane, srh_context::TvDefer &d, bool lists, bool strip, bool cert) {
	HIP_TRY(hipMemcpyAsync(d.host, lane.mem->cnt, sizeof(Counters), hipMemcpyDeviceToHost, lane.stream));
	if (lists) HIP_TRY(hipMemcpyAsync(d.span, lane.mem->span, 4*sizeof(int), hipMemcpyDeviceToHost, lane.stream));
	d.queued = true; d.lists = lists; d.strip = strip; d.cert = cert;
	return SRH_OK;
}

// what no pass of the lists repeats: the other view's "window fully usable" plane, the label table, the first capacities
int TvPass::lists_prepare(TvLists &S) const {
	int rc;
	if ((rc = lane.mem->band.lcount.ensure((size_t)(y1 - y0)*W))) return rc;
	ViewHost &O = c->views[oth];
	if ((rc = (sad || census) ? ensure_fulls(c, lane.stream, O, R) : ensure_full(c, lane.stream, O, R))) return rc;
	// the label-only part of pointFromDepth, once per pass instead of once per pixel and label
	if ((rc = lane.mem->band.tnum.ensure((size_t)p->num_depth_levels))) return rc;
	{ Scope s(c, lane.stream, "label_plane_table_kernel");
	  launch_label_plane_table(lane.stream, c->d_views, ref, *p, false, lane.mem->band.tnum); }
	// list capacity: the longest list seen so far on this context (hint); the FIRST time a guess from the geometry
	// (estimate_list_capacity: a few dozen curves' coarse polylines projected on the host -- round 5 ran a counting pass
	// there, twoview_count_kernel, 10 ms of a C5 pair's first call, and then sized the slots too tightly, so that the
	// pass was repeated: 104 ms for a pair whose steady state is 61).  A run that overflows its capacity is repeated
	// with the true maximum: the guess decides how long a pair's first call takes, never what it computes.
	int smax_guess = 0;
	S.cmax = c->list_cmax_hint;
	if (S.cmax <= 0 && c->list_count_pass) {
		HIP_TRY(hipMemsetAsync(lane.mem->span, 0, sizeof(int), lane.stream));
		{ Scope s(c, lane.stream, "twoview_count_kernel");
		  launch_twoview_count(lane.stream, c->d_views, ref, oth, W, *p, y0, y1 - y0, lane.mem->band.lcount, lane.mem->cnt, lane.mem->span, lane.mem->band.tnum); }
		int maxc = 0;
		if ((rc = read_back(lane.stream, &maxc, lane.mem->span, sizeof(int)))) return rc;
		S.cmax = std::max(8, (maxc + 7) & ~7);
	} else if (S.cmax <= 0) {
		estimate_list_capacity(c->views[ref].cam, O.cam, W, H, O.w, O.h, *p, y0, y1, S.cmax, smax_guess);
		S.guessed = true;
	}
	S.rows_mode = c->list_rows && W < 32768 && H < 32768;     // spans and row origins are stored as 16-bit signed
	if (c->views[ref].list_mode[oth] == 2) S.rows_mode = false;   // learnt: steep curves, list order is cheaper
	S.smax = c->list_smax_hint > 0 ? c->list_smax_hint : (S.guessed ? smax_guess : S.cmax + 64);
	return SRH_OK;
}

// one band of the row-run lists: list kernel, support windows beside it, cost, scan, the certified redo
int TvPass::lists_rows_band(const TvLists &S, int by, int nr) const {
	ViewHost &O = c->views[oth];
	int32_t *cnt_band = lane.mem->band.lcount + (size_t)(by - y0)*W;
	// the row-run cost kernel takes the pixels' constants (meanL, totalWeight, sum2, 1/totalWeight, SA) from the weights
	// kernel, which has the window in registers anyway, instead of making them on one lane in eight per tile
	double *pconst = (sad || census) ? nullptr : (double *)lane.mem->band.pconst;
	// The list kernel does not need the support windows, and its last waves drain for long (a wave walks
	// its 64 curves for ~2 ms): the windows are computed on a side stream queued behind it -- the geodesic
	// kernel's register-heavy waves only find room on a SIMD once the list kernel's have left it.
	if (!c->side_stream) {
		HIP_TRY(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&c->side_go, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&c->side_done, hipEventDisableTiming));
	}
	HIP_TRY(hipEventRecord(c->side_go, lane.stream));               // the window buffer's last readers are done by then
	{ Scope s(c, lane.stream, "twoview_rows_list_kernel");
	  launch_twoview_rows_list(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.lcand, S.cmax,
	                           cnt_band, lane.mem->band.lrowinfo, lane.mem->band.lmeta, S.smax, lane.mem->cnt, lane.mem->span, lane.mem->band.tnum); }
	if (c->side_weights) {
		HIP_TRY(hipStreamWaitEvent(c->side_stream, c->side_go, 0));
		run_weights(c, { c->side_stream, lane.mem }, ref, W, *p, by, nr, SRH_WTILE, pconst, true);
		HIP_TRY(hipEventRecord(c->side_done, c->side_stream));
		HIP_TRY(hipStreamWaitEvent(lane.stream, c->side_done, 0));
	} else run_weights(c, lane, ref, W, *p, by, nr, SRH_WTILE, pconst, true);
	if (S.cert) HIP_TRY(hipMemsetAsync(lane.mem->band.cflag, 0, sizeof(uint32_t), lane.stream));
	HIP_TRY(hipMemsetAsync(&lane.mem->cnt->strip_ticket, 0, 2*sizeof(unsigned int), lane.stream));   // the cost kernel's waves draw their tiles from it
	if (sad) {
		Scope s(c, lane.stream, "twoview_rows_sad_kernel");
		launch_twoview_rows_sad(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, O.fulls,
		                        lane.mem->band.lrowinfo, lane.mem->band.lmeta, lane.mem->band.cost, S.smax, lane.mem->cnt);
	} else if (census) {
		Scope s(c, lane.stream, "twoview_rows_census_kernel");
		launch_twoview_rows_census(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, O.fulls,
		                           lane.mem->band.lrowinfo, lane.mem->band.lmeta, lane.mem->band.cost, S.smax, lane.mem->cnt);
	} else {
		Scope s(c, lane.stream, "twoview_rows_cost_kernel");
		launch_twoview_rows_cost(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, O.full,
		                         lane.mem->band.lrowinfo, lane.mem->band.lmeta, lane.mem->band.cost, S.smax, lane.mem->cnt, S.cert ? (c->cert_form == 1 ? 5 : 3) : 0,
		                         pconst, S.cert && c->rows_masked ? O.tvp : nullptr, c->num_cus,
		                         c->rows_masked == 1 ? (const uint32_t *)(O.full + full_stat_offset((size_t)O.w*O.h)) : nullptr);
	}
	{ Scope s(c, lane.stream, "twoview_rows_scan_kernel");
	  launch_twoview_rows_scan(lane.stream, c->d_views, ref, oth, W, *p, by, nr, cnt_band, lane.mem->band.lcand, S.cmax,
	                           lane.mem->band.lrowinfo, lane.mem->band.lmeta, lane.mem->band.cost, S.smax, S.cert ? lane.mem->band.cflag : nullptr, -1, lane.mem->cnt, wout); }
	if (S.cert) {
		// certified arithmetic: the flagged pixels once more in the reference's arithmetic, launched for a capacity
		// (a list cut by a too small capacity is harmless here: the pass is repeated anyway)
		const int cap = redo_capacity((size_t)nr*W);
		{ Scope s(c, lane.stream, "twoview_rows_refill_kernel");
		  launch_twoview_rows_refill(lane.stream, W, O.w, *p, by, lane.mem->band.cflag, cap, lane.mem->band.wbuf, c->views[ref].tvp, O.tvp,
		                             lane.mem->band.lrowinfo, lane.mem->band.lmeta, lane.mem->band.cost, S.smax, lane.mem->cnt); }
		Scope s(c, lane.stream, "twoview_rows_rescan_kernel");
		launch_twoview_rows_scan(lane.stream, c->d_views, ref, oth, W, *p, by, nr, cnt_band, lane.mem->band.lcand, S.cmax,
		                         lane.mem->band.lrowinfo, lane.mem->band.lmeta, lane.mem->band.cost, S.smax, lane.mem->band.cflag, cap, lane.mem->cnt, wout);
	}
	winner_costs(by, nr, true);
	return SRH_OK;
}

// one pass of the lists with the capacities and in the mode of S: counters and maxima reset, buffers, every band queued
int TvPass::lists_pass(TvLists &S) const {
	int rc;
	HIP_TRY(hipMemsetAsync(lane.mem->cnt, 0, sizeof(Counters), lane.stream));
	HIP_TRY(hipMemsetAsync(lane.mem->span, 0, 4*sizeof(int), lane.stream));
	const bool rows_mode = S.rows_mode;
	const int ccap = rows_mode ? S.smax : S.cmax;                 // cost values per pixel
	// (row runs: the windows in the LDS-image layout, window rows padded to an even tap count -- the cost kernel's
	// waves fetch them by LDS-DMA)
	const size_t per_px = (size_t)(rows_mode ? (2*R + 1)*wimg_wp(R) : T)*sizeof(double) + (size_t)ccap*sizeof(double) + (size_t)S.cmax*sizeof(uint32_t)
	                      + (rows_mode ? (SRH_ROWS_NR + 1)*sizeof(uint32_t) : 0);
	const size_t lrows = S.lrows = rows_per_band(per_px);
	if ((rc = lane.mem->band.wbuf.ensure(rows_mode ? wimg_doubles(W, (int)lrows, R) : wbuf_doubles(W, (int)lrows, T)))) return rc;
	// row runs: lists and row tables are tiled per 64 pixels, cost slots per 32-pixel tile of a row
	const size_t px64 = (lrows*W + 63) & ~(size_t)63, px32 = lrows*(size_t)((W + 7)/8)*8;        /* (cost slots: tiles of 8 pixels) */
	if ((rc = lane.mem->band.cost.ensure((rows_mode ? px32 : lrows*W)*(size_t)ccap))) return rc;
	if ((rc = lane.mem->band.lcand.ensure((rows_mode ? px64 : lrows*W)*(size_t)S.cmax))) return rc;
	if (rows_mode && !sad && !census && (rc = lane.mem->band.pconst.ensure((lrows*(size_t)W + SRH_WTILE)*SRH_PC))) return rc;
	if (rows_mode) {
		if ((rc = lane.mem->band.lrowinfo.ensure(px64*(size_t)SRH_ROWS_NR))) return rc;
		if ((rc = lane.mem->band.lmeta.ensure(lrows*W))) return rc;
		if (S.cert && (rc = lane.mem->band.cflag.ensure(lrows*W + 1))) return rc;
		// NaN-bordered planes of both views: the general cost of the certified redo reads them without bound tests
		if (S.cert && ((rc = ensure_tvp(c, lane.stream, c->views[ref])) || (rc = ensure_tvp(c, lane.stream, c->views[oth])))) return rc;
	}
	for (int by = y0; by < y1; by += (int)lrows) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		const int nr = std::min((int)lrows, y1 - by);
		if (rows_mode) {
			if ((rc = lists_rows_band(S, by, nr))) return rc;
			continue;
		}
			int32_t *cnt_band = lane.mem->band.lcount + (size_t)(by - y0)*W;
			run_weights(c, lane, ref, W, *p, by, nr, SRH_WTILE);
			{ Scope s(c, lane.stream, "twoview_list_kernel");
			  launch_twoview_list(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.lcand, S.cmax,
			                      cnt_band, lane.mem->cnt, lane.mem->span, lane.mem->band.tnum); }
			if (sad) {
				Scope s(c, lane.stream, "twoview_list_sad_kernel");
				launch_twoview_list_sad(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf,
				                        cnt_band, lane.mem->band.lcand, lane.mem->band.cost, S.cmax, lane.mem->cnt);
			} else if (census) {
				Scope s(c, lane.stream, "twoview_list_census_kernel");
				launch_twoview_list_census(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf,
				                           cnt_band, lane.mem->band.lcand, lane.mem->band.cost, S.cmax, lane.mem->cnt);
			} else {
				Scope s(c, lane.stream, "twoview_list_cost_kernel");
				launch_twoview_list_cost(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, c->views[oth].full,
				                         cnt_band, lane.mem->band.lcand, lane.mem->band.cost, S.cmax, lane.mem->cnt);
			}
			{ Scope s(c, lane.stream, "twoview_list_scan_kernel");
			  launch_twoview_list_scan(lane.stream, c->d_views, ref, oth, W, *p, by, nr, cnt_band, lane.mem->band.lcand, lane.mem->band.cost, S.cmax, wout); }
			winner_costs(by, nr, false);
	}
	return SRH_OK;
}

// The candidate lists, with the capacity loop: a pass whose lists or cost slots overflowed is repeated with the measured
// maxima, a pair whose curves do not suit row runs in list order, a certified pass with more flagged pixels than the redo
// covers in the reference's arithmetic.  defer (srh_twoview_compute, a call's first attempt): a first row-run pass on
// learnt or guessed capacities is handed over unverified (defer->queued) instead of being waited for.
int TvPass::run_lists(bool cert_ok, srh_context::TvDefer *defer) const {
	int rc;
	TvLists S;
	if ((rc = lists_prepare(S))) return rc;
	for (int pass = 0; pass < 6; ++pass) {
		S.cert = S.rows_mode && cert_ok;
		if ((rc = lists_pass(S))) return rc;
		if (defer && pass == 0 && S.rows_mode &&
		    ((c->list_cmax_hint > 0 && c->list_smax_hint > 0 && c->views[ref].list_mode[oth] == 1) ||
		     (S.guessed && c->views[ref].list_mode[oth] == 0))) {
			// optimistic: capacities and path are those earlier runs of this pair learnt -- or, for a pair's FIRST call, the
			// host's guess and the row-run path -- (a pass that does not stand -- a longer list after a re-upload, say -- is
			// redone with the wait per pass)
			if ((rc = tv_defer_queue(lane, *defer, true, false, S.cert))) return rc;
			defer->cmax = S.cmax; defer->smax = S.smax;
			defer->guessed = S.guessed; defer->ref = ref; defer->oth = oth;
			if (c->debug_trace) fprintf(stderr, "[srh trace] lists %d>%d queued unverified: cmax %d smax %d guessed %d\n", ref, oth, S.cmax, S.smax, (int)S.guessed);
			c->stats.used_strip_kernel = 0;
			c->stats.used_dense_path = 0;
			HIP_TRY(hipGetLastError());
			return SRH_OK;
		}
		int mx[4] = { 0, 0, 0, 0 };
		if ((rc = read_back(lane.stream, mx, lane.mem->span, sizeof(mx)))) return rc;
		const int maxc = mx[0];
		if (c->debug_trace) fprintf(stderr, "[srh trace] lists %d>%d verified pass %d: cmax %d smax %d guessed %d -> longest list %d, slots %d, rows over %d\n",
		                            ref, oth, pass, S.cmax, S.smax, (int)S.guessed, mx[0], mx[1], mx[2]);
		if (S.rows_mode) {
			// a curve crossing more than SRH_ROWS_NR rows, or more slots than the 16-bit slot base
			// holds: this pair is evaluated in list order instead
			const int need = (mx[1] + 7) & ~7;
			if (mx[2] || need > 65528) {
				S.rows_mode = false; c->views[ref].list_mode[oth] = 2;
				if (maxc > S.cmax) S.cmax = (maxc + 7) & ~7;
				continue;
			}
			if (tv_lists_fit(mx, S.cmax, S.smax)) {
				Counters hc;
				if ((rc = read_back(lane.stream, &hc, lane.mem->cnt, sizeof(hc)))) return rc;
				tv_learn_lists(c, ref, oth, S.guessed, S.cmax, S.smax, mx, hc);
				if (hc.cert_overflow != 0) { cert_ok = false; continue; }   // more flagged pixels than the redo covers: mode 0
				if (S.cert) { c->stats.n_certified = (int64_t)hc.n_pixels; c->stats.n_flagged = (int64_t)hc.n_flagged; }
				break;
			}
			if (maxc > S.cmax) { S.cmax = (maxc + 7) & ~7; if (need <= S.smax) S.smax = std::max(S.smax, S.cmax + 64); }
			if (need > S.smax) S.smax = need;
			S.guessed = false;                                    // (the repeat runs on measured maxima)
			continue;
		}
		if (maxc <= S.cmax) {
			const int cm = S.guessed ? std::max(8, (maxc + 7) & ~7) : S.cmax;
			if (cm > c->list_cmax_hint) c->list_cmax_hint = cm;
			break;
		}
		S.cmax = (maxc + 7) & ~7;                                 // hint too small: repeat with the true maximum
		S.guessed = false;
	}
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

// ---- the dense plan (row-aligned rig): cost rows by the persistent strip kernel (srh_strip.hip, cost_sad:
// srh_sad_strip.hip) or by one workgroup per tile, then the scan over them

// What an attempt of the dense plan queues before its bands: label table, scan template, band buffers, the views' padded
// planes.  D.strip falls back to the per-tile kernel for thin bands: the strip kernel wants dozens of tiles per
// persistent workgroup and launch (option strip = 4 / 8 forces it for tests)
int TvPass::dense_prepare(TvDense &D) const {
	int rc;
	D.tscan = c->tscan != 0;
	if ((rc = lane.mem->band.tnum.ensure((size_t)p->num_depth_levels + 8))) return rc;   // (+ 8: the template scan reads the table in whole eights)
	if (D.tscan && (rc = lane.mem->band.stpl.ensure(scan_template_bytes()))) return rc;
	// (option side_weights: the first band queues them on the side stream, behind its windows kernel -- dense_band_inputs)
	D.tables_pending = c->side_weights != 0;
	D.tpl_wait = false;
	if (!D.tables_pending) dense_tables(lane, D, true, true);
	for (int pass = 0; pass < 2; ++pass) {
		const int wdoubles = D.strip ? (2*R + 1)*wimg_wp(R) : T;    // doubles per pixel window in the band buffer
		D.rows = rows_per_band((size_t)wdoubles*sizeof(double) + (size_t)D.cstride*sizeof(double));
		if (D.strip && !strip_only && c->strip == 1 && (size_t)((W + SRH_WTILE - 1)/SRH_WTILE)*D.rows < (size_t)48*2*c->num_cus) D.strip = false;
		else break;
	}
	const size_t rows = D.rows;
	if ((rc = lane.mem->band.wbuf.ensure(D.strip ? wimg_doubles(W, (int)rows, R) : wbuf_doubles(W, (int)rows, T)))) return rc;
	if ((rc = lane.mem->band.cost.ensure(rows*(size_t)((W + 31)/32)*32*(size_t)D.cstride))) return rc;   // 32-pixel tiles
	// (+ one tile of slack: the strip kernel copies whole 32-pixel pieces of these rows)
	if ((rc = lane.mem->band.pconst.ensure((rows*(size_t)W + SRH_WTILE)*SRH_PC))) return rc;
	if ((rc = lane.mem->band.prange.ensure(rows*(size_t)W + SRH_WTILE))) return rc;
	if (!strip_only && (rc = lane.mem->band.filllist.ensure(rows*(size_t)W + 1))) return rc;    // (capacity: the band's pixels)
	if (D.tscan && (rc = lane.mem->band.tileflag.ensure(rows*(size_t)((W + 63)/64) + 1))) return rc;
	if (D.cert && (rc = lane.mem->band.cflag.ensure(rows*(size_t)W + 1))) return rc;
	D.lanes = D.strip ? strip_block_lanes(D.cstride, c->strip == 1 ? 0 : c->strip) : 8;
	// NaN-bordered gray_tv planes of both views (strip kernel; the general cost of the left-out columns and of the
	// certified redo on either dense path)
	if ((rc = ensure_tvp(c, lane.stream, c->views[ref])) || (rc = ensure_tvp(c, lane.stream, c->views[oth]))) return rc;
	if (D.strip && sad) {
		if ((rc = ensure_sad_planes(c, lane.stream, c->views[oth], R))) return rc;
	} else if (D.strip && census) {
		if ((rc = ensure_census_planes(c, lane.stream, ref, R)) || (rc = ensure_census_planes(c, lane.stream, oth, R))) return rc;
	} else if (D.strip) {
		// zero-bordered "window fully usable" plane of the other view
		ViewHost &O = c->views[oth];
		if (!O.fullp) HIP_TRY(O.fullp.alloc(padded_size(O.w, O.h)));
		if (O.fullp_r != R) {
			Scope s(c, lane.stream, "padded_full_kernel");
			launch_padded_full(lane.stream, O.gray_tv, O.w, O.h, R, O.fullp);
			O.fullp_r = R;
		}
	}
	return SRH_OK;
}

// the label-only part of the pinhole walk and the pass's candidate template: the reference's walk at one pixel
// (srh_dense.hip, "template scan")
void TvPass::dense_tables(const Lane &on, const TvDense &D, bool table, bool tpl) const {
	if (table) {
		Scope s(c, on.stream, "pinhole_label_table_kernel");
		launch_pinhole_label_table(on.stream, c->d_views, ref, *p, false, on.mem->band.tnum);
	}
	if (tpl && D.tscan) {
		Scope s(c, on.stream, "twoview_template_kernel");
		launch_scan_template(on.stream, c->d_views, ref, oth, *p, y0, y1 - y0, on.mem->band.tnum, on.mem->band.stpl);
	}
}

// the cost kernel's form under `arith`: its blocks start on even columns (what the fill launch and the fill list go by)
bool TvPass::dense_fill_padded(const TvDense &D, int arith) const { return D.strip ? D.lanes == 8 : arith != 5; }

// A band's support windows (with the pixels' constants for cost_ncc), the pixels' column ranges and the list of the pixels
// whose last columns the cost kernel under `arith` leaves out.
// Option side_weights: the windows kernel is queued first, on the pass's stream; label table, range kernel and scan
// template (table and template: the first band's) run on the context's side stream -- one stream for both passes of
// srh_twoview_compute, in order, each band waiting (side_go) for what its pass's stream held when the band began: the last
// readers of the tables and ranges it overwrites.  The pass's stream takes table and ranges back (side_done) before the
// cost kernel, the template (side_tpl) before the first scan: table and range kernel find room on a compute unit beside the
// windows kernel's waves, the template's workgroup (80 registers per lane, 45 KB of LDS) does not and starts when the
// windows kernel leaves -- behind the range kernel it holds nothing up (profiles/dense_tail_timeline.txt).
int TvPass::dense_band_inputs(TvDense &D, int by, int nr, int arith) const {
	uint32_t *filllist = strip_only ? nullptr : (uint32_t *)lane.mem->band.filllist;
	const bool side = c->side_weights != 0;
	if (side) {
		if (!c->side_stream) {
			HIP_TRY(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
			HIP_TRY(hipEventCreateWithFlags(&c->side_go, hipEventDisableTiming));
			HIP_TRY(hipEventCreateWithFlags(&c->side_done, hipEventDisableTiming));
		}
		if (!c->side_tpl) HIP_TRY(hipEventCreateWithFlags(&c->side_tpl, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(c->side_go, lane.stream));
	}
	run_weights(c, lane, ref, W, *p, by, nr, SRH_WTILE, !strip_only ? (double *)lane.mem->band.pconst : nullptr, D.strip);
	const bool tables = side && D.tables_pending;
	D.tables_pending = false;
	// where table, ranges and template are made: the pass's scratch, on the side stream or on the pass's own
	const Lane on = { side ? c->side_stream : lane.stream, lane.mem };
	if (side) {
		HIP_TRY(hipStreamWaitEvent(on.stream, c->side_go, 0));
		if (tables) dense_tables(on, D, true, false);
	}
	hipError_t e = filllist ? hipMemsetAsync(filllist, 0, sizeof(uint32_t), on.stream) : hipSuccess;
	{ Scope s(c, on.stream, "pixel_range_kernel");
	  launch_pixel_range(on.stream, c->d_views, ref, oth, W, *p, by, nr, on.mem->band.tnum, D.cstride, on.mem->band.prange,
	                     D.lanes, dense_fill_padded(D, arith), filllist); }
	if (side) {
		if (e == hipSuccess) e = hipEventRecord(c->side_done, on.stream);
		if (tables && D.tscan) {
			dense_tables(on, D, false, true);
			if (e == hipSuccess) e = hipEventRecord(c->side_tpl, on.stream);
			D.tpl_wait = true;
		}
		if (e == hipSuccess) e = hipStreamWaitEvent(lane.stream, c->side_done, 0);
	}
	if (e != hipSuccess) return fail(SRH_E_DEVICE, "dense band inputs: %s", hipGetErrorString(e));
	return SRH_OK;
}

// the band's cost rows under one arithmetic: strip kernel or one workgroup per tile, then the left-out columns
// (raw, diagnostics: the certified strip forms without the in-kernel exact redo)
int TvPass::dense_cost_pass(const TvDense &D, int by, int nr, int arith, bool raw) const {
	const int cstride = D.cstride;
	const size_t wstride = SRH_WTILE;
	if (sad) {
		// (every column of [lo, hi] is written: no fill launch, which would evaluate cost_ncc)
		HIP_TRY(hipMemsetAsync(&lane.mem->cnt->strip_ticket, 0, 2*sizeof(unsigned int), lane.stream));
		Scope s(c, lane.stream, "twoview_strip_sad_kernel");
		if (!launch_twoview_strip_sad(lane.stream, W, H, *p, by, nr, lane.mem->band.wbuf, lane.mem->band.prange, c->views[ref].tvp,
		                              c->views[oth].grayp, c->views[oth].fullsp, lane.mem->band.cost, cstride, lane.mem->cnt, c->num_cus))
			return fail(SRH_E_UNSUPPORTED, "twoview_strip_sad_kernel: no instantiation for radius %d", R);
		return SRH_OK;
	}
	if (census) {
		// (likewise: every column of [lo, hi] is written)
		HIP_TRY(hipMemsetAsync(&lane.mem->cnt->strip_ticket, 0, 2*sizeof(unsigned int), lane.stream));
		Scope s(c, lane.stream, "twoview_strip_census_kernel");
		if (!launch_twoview_strip_census(lane.stream, W, H, *p, by, nr, lane.mem->band.wbuf, lane.mem->band.prange, c->views[ref].cenrefp,
		                                 c->views[oth].cenothp, c->views[oth].fullsp, lane.mem->band.cost, cstride, lane.mem->cnt, c->num_cus))
			return fail(SRH_E_UNSUPPORTED, "twoview_strip_census_kernel: no instantiation for radius %d", R);
		return SRH_OK;
	}
	if (D.strip) {
		HIP_TRY(hipMemsetAsync(&lane.mem->cnt->strip_ticket, 0, 2*sizeof(unsigned int), lane.stream));
		{ Scope s(c, lane.stream, "twoview_strip_cost_kernel");
		  launch_twoview_strip_cost(lane.stream, c->d_views, ref, oth, W, H, *p, by, nr, lane.mem->band.wbuf, lane.mem->band.pconst, lane.mem->band.prange,
		                            c->views[ref].tvp, c->views[oth].tvp, c->views[oth].fullp, lane.mem->band.cost, cstride,
		                            lane.mem->cnt, arith, c->num_cus, D.lanes, raw); }
	} else {
		{ Scope s(c, lane.stream, "twoview_dense_cost_kernel");
		  if (arith == 2)
			launch_twoview_dense_cost_f32(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, wstride,
			                              lane.mem->band.tnum, lane.mem->band.cost, cstride, lane.mem->cnt, lane.mem->band.pconst, c->f32_form);
		  else
			launch_twoview_dense_cost(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, wstride,
			                          lane.mem->band.tnum, lane.mem->band.cost, cstride, lane.mem->cnt, lane.mem->band.pconst, arith, lane.mem->band.prange); }
	}
	// the left-out columns (per-tile kernel: its one-pass form leaves none out; D.lanes is 8 there), from the list the range
	// kernel made for this form
	Scope s(c, lane.stream, "twoview_lazy_fill_kernel");
	launch_twoview_lazy_fill(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.prange, lane.mem->band.filllist, lane.mem->band.wbuf, wstride, c->views[ref].tvp,
	                         c->views[oth].tvp, D.strip, D.lanes, dense_fill_padded(D, arith), lane.mem->band.cost, cstride, lane.mem->cnt);
	return SRH_OK;
}

// one attempt of the dense plan: every band queued; the counters say whether it stands (tv_dense_verdict)
int TvPass::run_dense(TvDense &D) const {
	int rc;
	if ((rc = dense_prepare(D))) return rc;
	// (the strip kernel's certified form: 5 = one sweep over the window, 3 = the reference's two sweeps fused; option "cert_form")
	const int cost_arith = c->arith == 3 ? (D.cert ? (c->cert_form == 1 ? 5 : 3) : 0) : c->arith;
	for (int by = y0; by < y1; by += (int)D.rows) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		const int nr = std::min((int)D.rows, y1 - by);
		if ((rc = dense_band_inputs(D, by, nr, cost_arith))) return rc;
		if (D.cert) HIP_TRY(hipMemsetAsync(lane.mem->band.cflag, 0, sizeof(uint32_t), lane.stream));
		if ((rc = dense_cost_pass(D, by, nr, cost_arith, false))) return rc;
		if (D.tpl_wait) { HIP_TRY(hipStreamWaitEvent(lane.stream, c->side_tpl, 0)); D.tpl_wait = false; }
		{ Scope s(c, lane.stream, "twoview_scan_kernel");
		  launch_twoview_scan(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.tnum, lane.mem->band.cost, D.cstride, lane.mem->cnt, lane.mem->band.prange,
		                      D.cert ? lane.mem->band.cflag : nullptr, -1, D.cert && D.strip ? lane.mem->band.pconst : nullptr, D.tscan ? lane.mem->band.stpl : nullptr, lane.mem->band.tileflag, c->num_cus, wout, c->tscan_bound); }
		if (D.cert) {
			// the pixels whose decisions the bound does not cover, in the reference's arithmetic: their cost rows are
			// refilled and they are scanned again -- launched for a capacity, the count stays on the device
			// (one kernel does both where the wave form of the rescan is eligible: twoview_redo_kernel, the columns beside the walk)
			const int cap = redo_capacity((size_t)nr*W);
			if (twoview_redo_takes(*p, D.cstride)) {
				Scope s(c, lane.stream, "twoview_redo_kernel");
				launch_twoview_redo(lane.stream, c->d_views, ref, oth, W, *p, by, lane.mem->band.tnum, lane.mem->band.wbuf, D.strip, c->views[ref].tvp,
				                    c->views[oth].tvp, lane.mem->band.cost, D.cstride, lane.mem->band.prange, lane.mem->band.cflag, cap, lane.mem->cnt, wout);
			} else {
				{ Scope s(c, lane.stream, "twoview_refill_kernel");
				  launch_twoview_refill(lane.stream, W, *p, by, lane.mem->band.prange, lane.mem->band.cflag, cap, lane.mem->band.wbuf, D.strip, c->views[ref].tvp,
				                        c->views[oth].tvp, lane.mem->band.cost, D.cstride, lane.mem->cnt); }
				Scope s(c, lane.stream, "twoview_rescan_kernel");
				launch_twoview_scan(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.tnum, lane.mem->band.cost, D.cstride, lane.mem->cnt, lane.mem->band.prange,
				                    lane.mem->band.cflag, cap, nullptr, nullptr, nullptr, c->num_cus, wout);
			}
		}
		winner_costs(by, nr, D.strip);
	}
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

// what the counters of a dense attempt say: the result stands only if no candidate left its row / column range
enum TvVerdict { TV_STANDS, TV_STRIP_OVERFLOW, TV_CERT_OVERFLOW, TV_NOT_ROW_ALIGNED };
static TvVerdict tv_dense_verdict(const Counters &h, bool strip) {
	if (strip && h.strip_overflow != 0) return TV_STRIP_OVERFLOW;   // a tile's ranges did not fit one LDS chunk
	if (h.cert_overflow != 0) return TV_CERT_OVERFLOW;              // more flagged pixels than the redo covers
	return h.not_row_aligned == 0 ? TV_STANDS : TV_NOT_ROW_ALIGNED;
}

// ---- the last resort: the one-thread-per-pixel walk kernel, which visits every point of every curve
int TvPass::run_walk() const {
	int rc;
	const int rows = (int)rows_per_band((size_t)T*sizeof(double));
	if ((rc = lane.mem->band.wbuf.ensure(wbuf_doubles(W, rows, T)))) return rc;
	for (int by = y0; by < y1; by += rows) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		const int nr = std::min(rows, y1 - by);
		run_weights(c, lane, ref, W, *p, by, nr, SRH_WTILE);
		{ Scope s(c, lane.stream, "twoview_generic_kernel");
		  launch_twoview_generic(lane.stream, c->d_views, ref, oth, W, *p, by, nr, lane.mem->band.wbuf, SRH_WTILE, lane.mem->cnt, kind, wout); }
		winner_costs(by, nr, false);
	}
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

// The controller: the plan's first choice, then at most four attempts, each read by its counters -- a strip overflow takes
// the per-tile kernel (cost_sad and the census cost, which have the strip form only: the candidate lists), a certified pass with more flagged
// pixels than its redo covers the reference's arithmetic, a dense plan the device refutes the general kernels.  On a
// call's first attempt srh_twoview_compute's passes (defer) are handed over unverified instead.
// (a HIP error or a refused band buffer returns straight out: with_thinner_bands retries the whole call)
static int twoview_wta_run(srh_context *c, const Lane &lane, srh_context::TvDefer *first_defer, int ref, int oth, const srh_params *p, int y0, int y1) {
	int rc;
	TvPass P;
	if ((rc = tv_pass_init(P, c, lane, ref, oth, p, y0, y1))) return rc;
	if (P.y1 <= P.y0) return SRH_OK;
	if ((rc = ensure_wta_planes(c, lane.stream, ref, oth))) return rc;
	// (srh_twoview_compute made both views' signatures before its streams forked: nothing is queued here then)
	if (P.census && ((rc = ensure_census(c, lane.stream, ref)) || (rc = ensure_census(c, lane.stream, oth)))) return rc;
	P.wout = c->wta_keep() ? (int32_t *)c->views[ref].wta_xy : nullptr;
	if (c->subpixel) {
		// the label-only part of pointFromDepth for the neighbours kernel's walk (a buffer of its own: band.tnum holds
		// whatever table the pass's own path reads)
		if ((rc = lane.mem->band.subpx_tdist.ensure((size_t)p->num_depth_levels))) return rc;
		Scope s(c, lane.stream, "label_plane_table_kernel");
		launch_label_plane_table(lane.stream, c->d_views, ref, *p, false, lane.mem->band.subpx_tdist);
		P.subpx_tdist = lane.mem->band.subpx_tdist;
	}
	const TvPlan plan = P.plan();

	c->last_fused = false;
	if (plan.fused) {
		bool stands = false;
		if ((rc = P.run_fused(stands))) return rc;
		if (stands) {
			c->stats.used_dense_path = 1;
			c->last_fused = true;
			return SRH_OK;
		}
	}

	bool dense = plan.dense;
	TvDense D;
	D.cstride = plan.cstride;
	// the persistent strip form of the cost kernel: exact / fma arithmetic, candidate ranges of a 32-pixel tile inside one
	// LDS chunk; anything else, or a range that turns out wider, takes the per-tile kernel
	D.strip = dense && (P.strip_only || (c->strip != 0 && c->arith != 2)) && plan.cstride + SRH_WTILE <= strip_chunk_columns();
	// (strip_select_block, the strip kernel's blocked select form, drops an unusable tap by multiplying with 0.0 and needs
	// finite weights for it; geodesic_sigma <= 0 gives the taps outside the image, which keep geodesic_init, the weight
	// +inf or NaN: such a pass takes the per-tile kernel, whose select forms are true selects)
	if (!P.strip_only && p->weight_kind == SRH_WEIGHT_GEODESIC && !(p->geodesic_sigma > 0)) D.strip = false;
	// certified arithmetic (arith = 3, the default): fused cost loops in the strip kernel + the certified scan; where the
	// strip kernel does not run, or the parameters leave the bound no room, the reference's arithmetic
	bool cert_ok = c->arith == 3 && !P.sad && !P.census && cert_bound(*p).ok != 0;
	c->stats.n_certified = c->stats.n_flagged = 0;
	// (a negative wta_margin -- not the reference's: its margin is the constant +1e-10, twoviewstereo.cpp:293 -- makes a
	// revisited winner beat itself, so the candidate lists' dropped joint duplicates would matter: the walk kernel, which
	// visits every point, takes such a run)
	const bool lists = !c->force_walk && P.R <= 5 && P.W < 65536 && P.H < 65536 && p->wta_margin >= 0;
	for (int attempt = 0; attempt < 4; ++attempt) {
		HIP_TRY(hipMemsetAsync(lane.mem->cnt, 0, sizeof(Counters), lane.stream));
		srh_context::TvDefer *defer = attempt == 0 ? first_defer : nullptr;
		if (!dense) {
			if ((rc = lists ? P.run_lists(cert_ok, defer) : P.run_walk())) return rc;
			if (lists && defer && defer->queued) return SRH_OK;
			break;
		}
		D.cert = cert_ok;
		if ((rc = P.run_dense(D))) return rc;
		if (defer) {
			if ((rc = tv_defer_queue(lane, *defer, false, D.strip, cert_ok))) return rc;
			c->stats.used_strip_kernel = D.strip ? 1 : 0;
			c->stats.used_dense_path = 1;
			return SRH_OK;
		}
		Counters hc;
		if ((rc = read_back(lane.stream, &hc, lane.mem->cnt, sizeof(hc)))) return rc;
		const TvVerdict v = tv_dense_verdict(hc, D.strip);
		if (v == TV_STRIP_OVERFLOW) { D.strip = false; if (P.strip_only) dense = false; continue; }
		if (v == TV_CERT_OVERFLOW) { cert_ok = false; continue; }
		c->stats.n_certified = (int64_t)hc.n_certified; c->stats.n_flagged = (int64_t)hc.n_flagged;
		if (v == TV_STANDS) break;
		dense = false;                                            // redo with the general kernels
		D.strip = false;
	}
	c->stats.used_strip_kernel = D.strip ? 1 : 0;
	c->stats.used_dense_path = dense ? 1 : 0;
	return SRH_OK;
}

extern "C" int srh_twoview_wta(srh_context *c, int ref, int oth, const srh_params *p, int y0, int y1) {
	int rc;
	if ((rc = check_slot(c, ref, true)) || (rc = check_slot(c, oth, true)) || (rc = check_params(p))) return rc;
	return with_thinner_bands(c, [&] { return twoview_wta_run(c, c->main_lane(), nullptr, ref, oth, p, y0, y1); });
}

// Diagnostic (tests/test_gpu_cert_rows.py): the cost rows of rows [y0, y1) on the row-aligned dense plan, straight from the
// cost kernel -- what the scan would look up.  form: 0 the reference's arithmetic, 3 two fused sweeps, 5 one-pass (the
// certified forms), 1 fused unchecked, 2 the single-precision kernel (srh_dense_f32.hip, option f32_form; per tile whatever
// option strip says); raw != 0: without the in-kernel exact redo (uncertified candidates are NaN).  The plan and the
// preparation are the pass's (tv_plan, tv_dense_prepare); the rows have to fit one band, whose cost pass runs alone.
extern "C" int srh_twoview_cost_rows(srh_context *c, int ref, int oth, const srh_params *p, int y0, int y1, int form, int raw,
                                     double *cost_out, size_t cost_doubles, int32_t *range_out, int *cstride_out, int *used_strip)
{
	int rc;
	if ((rc = check_slot(c, ref, true)) || (rc = check_slot(c, oth, true)) || (rc = check_params(p))) return rc;
	if (form != 0 && form != 3 && form != 5 && form != 1 && form != 2) return fail(SRH_E_INVALID, "form must be 0, 1, 2, 3 or 5");
	if ((form == 3 || form == 5) && !cert_bound(*p).ok) return fail(SRH_E_UNSUPPORTED, "the parameters leave the error bound no room");
	const bool sad = c->cost_kind == SRH_COST_SAD, census = c->cost_kind == SRH_COST_CENSUS;
	const bool strip_only = sad || census;
	if (census && !c->census_dense) return fail(SRH_E_UNSUPPORTED, "cost rows of the census cost exist on the dense plan only (option census_dense)");
	if (sad && !c->sad_dense) return fail(SRH_E_UNSUPPORTED, "cost rows of cost_sad exist on the dense plan only (option sad_dense)");
	if (strip_only && form != 0) return fail(SRH_E_INVALID, "cost_sad and the census cost have one arithmetic only: form must be 0");
	TvPass P;
	if ((rc = tv_pass_init(P, c, c->main_lane(), ref, oth, p, y0, y1))) return rc;
	const TvPlan plan = P.plan();
	if (P.y1 <= P.y0 || !plan.dense)
		return fail(SRH_E_UNSUPPORTED, "cost rows exist on the row-aligned dense plan only (radius 5 or 2, rectified pinhole pair)");
	c->last_fused = false;
	c->stats.n_certified = c->stats.n_flagged = 0;
	HIP_TRY(hipMemsetAsync(c->mem.cnt, 0, sizeof(Counters), c->stream));
	TvDense D;
	D.cstride = plan.cstride;
	D.strip = (strip_only || c->strip != 0) && plan.cstride + SRH_WTILE <= strip_chunk_columns();
	if (!strip_only && p->weight_kind == SRH_WEIGHT_GEODESIC && !(p->geodesic_sigma > 0)) D.strip = false;   // (as in the pass: finite weights only)
	D.cert = form != 0 && !strip_only && cert_bound(*p).ok != 0;
	if (form == 2) D.strip = D.cert = false;                      // (the f32 kernel is a per-tile kernel, as in the pass under arith = 2)
	if ((rc = P.dense_prepare(D))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	const int nr = std::min((int)D.rows, P.y1 - P.y0);
	if ((rc = P.dense_band_inputs(D, P.y0, nr, form))) return rc;
	if (nr != P.y1 - P.y0) return fail(SRH_E_UNSUPPORTED, "cost rows: the rows asked for do not fit one band (%d of %d)", nr, P.y1 - P.y0);
	if (cost_out) {
		// the band's cost rows under the arithmetic asked for, as the cost kernel leaves them, and the pixels' column ranges
		const size_t nd = (size_t)nr*((P.W + 31)/32)*32*(size_t)D.cstride;
		if (cost_doubles < nd) return fail(SRH_E_INVALID, "cost rows: buffer of %zu doubles, %zu needed", cost_doubles, nd);
		HIP_TRY(hipMemsetAsync(c->mem.band.cost, 0xff, nd*sizeof(double), c->stream));   // (never-written entries read as a NaN with payload -1)
		if ((rc = P.dense_cost_pass(D, P.y0, nr, form, raw != 0))) return rc;
		HIP_TRY(hipMemcpyAsync(cost_out, c->mem.band.cost, nd*sizeof(double), hipMemcpyDeviceToHost, c->stream));
		if (range_out) HIP_TRY(hipMemcpyAsync(range_out, c->mem.band.prange, (size_t)nr*P.W*sizeof(PixRange), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	if (cstride_out) *cstride_out = D.cstride;
	if (used_strip) *used_strip = D.strip ? 1 : 0;
	return SRH_OK;
}

// cost_sad / cost_ncc of arbitrary pairs (the host classes' protected cost_sad / cost_ncc, tests): the support window of
// (x1, y1) built on the device, the reference-form costs of srh_walk.hpp; synchronous, host pointers
extern "C" int srh_twoview_pair_costs(srh_context *c, int ref, int oth, const srh_params *p, int kind, int n,
                                      const int32_t *xy, double *out)
{
	int rc;
	if ((rc = check_slot(c, ref, true)) || (rc = check_slot(c, oth, true)) || (rc = check_params(p))) return rc;
	if (kind != SRH_COST_NCC && kind != SRH_COST_SAD && kind != SRH_COST_CENSUS)
		return fail(SRH_E_INVALID, "kind must be SRH_COST_NCC, SRH_COST_SAD or SRH_COST_CENSUS");
	if (n < 0 || (n > 0 && (!xy || !out))) return fail(SRH_E_INVALID, "null pairs or output");
	if (p->window_radius > 5) return fail(SRH_E_UNSUPPORTED, "pair costs take window radii up to 5");
	if (n == 0) return SRH_OK;
	const ViewHost &L = c->views[ref];
	for (int k = 0; k < n; ++k)
		if (xy[4*k] < 0 || xy[4*k + 1] < 0 || xy[4*k] >= L.w || xy[4*k + 1] >= L.h)
			return fail(SRH_E_INVALID, "pair %d: reference pixel (%d, %d) outside the %dx%d view", k, xy[4*k], xy[4*k + 1], L.w, L.h);
	HIP_TRY(hipSetDevice(c->device));
	if (kind == SRH_COST_CENSUS && ((rc = ensure_census(c, c->stream, ref)) || (rc = ensure_census(c, c->stream, oth)))) return rc;
	DevBuf<int32_t> dxy; DevBuf<double> dout;
	HIP_TRY(dxy.alloc((size_t)4*n));
	HIP_TRY(dout.alloc((size_t)n));
	HIP_TRY(hipMemcpyAsync(dxy, xy, (size_t)4*n*sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
	{ Scope s(c, c->stream, "pair_costs_kernel");
	  launch_pair_costs(c->stream, c->d_views, ref, oth, *p, kind, n, dxy, dout); }
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	dxy.free(); dout.free();
	return SRH_OK;
}

// the census signature plane of a view (w*h words), made if the slot does not hold it yet; synchronous, host pointer
extern "C" int srh_view_census(srh_context *c, int slot, uint64_t *out) {
	int rc;
	if ((rc = check_slot(c, slot, true))) return rc;
	if (!out) return fail(SRH_E_INVALID, "null output");
	HIP_TRY(hipSetDevice(c->device));
	if ((rc = ensure_census(c, c->stream, slot))) return rc;
	HIP_TRY(hipGetLastError());
	const ViewHost &v = c->views[slot];
	HIP_TRY(hipMemcpyAsync(out, v.census, (size_t)v.w*v.h*sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

extern "C" int srh_debug_exp(srh_context *c, const double *x, int n, double *kernel_out, double *library_out) {
	if (!c || !x || !kernel_out || !library_out || n < 1) return fail(SRH_E_INVALID, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	DevBuf<double> d;
	HIP_TRY(d.alloc((size_t)n*3));
	hipError_t e = hipMemcpyAsync(d, x, (size_t)n*sizeof(double), hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) {
		launch_geo_exp_probe(c->stream, d, n, d + n, d + 2*(size_t)n);
		e = hipMemcpyAsync(kernel_out, d + n, (size_t)n*sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess) e = hipMemcpyAsync(library_out, d + 2*(size_t)n, (size_t)n*sizeof(double), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	d.free();
	if (e != hipSuccess) return fail(SRH_E_DEVICE, "srh_debug_exp: %s", hipGetErrorString(e));
	return SRH_OK;
}

extern "C" int srh_twoview_cross_check(srh_context *c, int left, int right, const srh_params *p) {
	int rc;
	if ((rc = check_slot(c, left, true)) || (rc = check_slot(c, right, true)) || (rc = check_params(p))) return rc;
	const ViewHost &L = c->views[left], &Rv = c->views[right];
	if (L.w != Rv.w || L.h != Rv.h) return fail(SRH_E_INVALID, "TwoViewStereo needs equal-sized views");
	HIP_TRY(hipSetDevice(c->device));
	// left pass completes (stream order) before the right pass reads the filtered left map
	{ Scope s(c, c->stream, "twoview_cross_check_kernel"); launch_twoview_cross_check(c->stream, c->d_views, left, right, L.w, L.h, *p); }
	{ Scope s(c, c->stream, "twoview_cross_check_kernel"); launch_twoview_cross_check(c->stream, c->d_views, right, left, L.w, L.h, *p); }
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

static bool tv_pass_stands(const srh_context::TvDefer &d) {
	const Counters &h = *d.host;
	if (d.lists) return tv_lists_fit(d.span, d.cmax, d.smax) && h.cert_overflow == 0;
	return tv_dense_verdict(h, d.strip) == TV_STANDS;
}

static int twoview_filter(srh_context *c, int left, int right, const srh_params *p);
static int check_filter(srh_context *c, int slot, const srh_params *p, int flags);
static int twoview_speckles(srh_context *c, int left, int right, const srh_params *p);
static int check_twoview_speckles(srh_context *c, int left, int right, const srh_params *p);

extern "C" int srh_twoview_compute(srh_context *c, int left, int right, const srh_params *p,
                                   double *left_out, double *right_out)
{
	int rc;
	if ((rc = check_slot(c, left, true)) || (rc = check_slot(c, right, true)) || (rc = check_params(p))) return rc;
	// option "filter_invalid": what the hole filling refuses is refused before any launch, not after the two passes
	if (c->filter_invalid && ((rc = check_filter(c, left, p, c->filter_invalid)) || (rc = check_filter(c, right, p, c->filter_invalid)))) return rc;
	if (c->speckle_min_size && (rc = check_twoview_speckles(c, left, right, p))) return rc;
	// the maps go to the host early only when nothing rewrites them after the cross-check
	const bool tail = c->filter_invalid || c->speckle_min_size;
	HIP_TRY(hipSetDevice(c->device));
	for (auto &d : c->tv_defer) {
		if (!d.host) HIP_TRY(hipHostMalloc((void **)&d.host, sizeof(Counters)));
		if (!d.span) HIP_TRY(hipHostMalloc((void **)&d.span, 4*sizeof(int)));
		d.queued = false; d.lists = false; d.guessed = false;
	}
	if (c->tv_overlap) {
		srh_context::TvSlot &T = c->tv_slot;
		if (!T.stream) {
			HIP_TRY(hipStreamCreateWithFlags(&T.stream, hipStreamNonBlocking));
			HIP_TRY(hipEventCreateWithFlags(&T.go, hipEventDisableTiming));
			HIP_TRY(hipEventCreateWithFlags(&T.done, hipEventDisableTiming));
			HIP_TRY(T.mem.cnt.alloc(1));
			HIP_TRY(T.mem.span.alloc(4));
		}
		// the NaN-bordered planes both passes read (tv_dense_prepare makes them on demand, on its own stream) exist at `go`
		// (and so do the census signatures of both views)
		if (c->cost_kind == SRH_COST_CENSUS && ((rc = ensure_census(c, c->stream, left)) || (rc = ensure_census(c, c->stream, right)))) return rc;
		if (c->cost_kind == SRH_COST_SAD && c->sad_dense && (p->window_radius == 5 || p->window_radius == 2))
			for (int k = 0; k < 2; ++k)
				if ((rc = ensure_sad_planes(c, c->stream, c->views[k == 0 ? left : right], p->window_radius))) return rc;
		if (c->cost_kind == SRH_COST_CENSUS && c->census_dense && (p->window_radius == 5 || p->window_radius == 2))
			for (int k = 0; k < 2; ++k)
				if ((rc = ensure_census_planes(c, c->stream, k == 0 ? left : right, p->window_radius))) return rc;
		if ((p->window_radius == 5 || p->window_radius == 2) &&
		    ((rc = ensure_tvp(c, c->stream, c->views[left])) || (rc = ensure_tvp(c, c->stream, c->views[right])))) return rc;
		// (and the WTA by-products' planes of both views, option "wta_outputs", are allocated and hold their "none" values there)
		if ((rc = ensure_wta_planes(c, c->stream, left, right)) || (rc = ensure_wta_planes(c, c->stream, right, left))) return rc;
		HIP_TRY(hipEventRecord(T.go, c->stream));
	}
	// progress steps as TwoViewStereo emits them (twoviewstereo.cpp:234,405,597,225)
	progress(c, 1, "Computing cost volume for left image...");
	// (a pass whose verdict may wait: twoview_wta_run hands it over through tv_defer[k])
	auto deferred_wta = [&](int k, const Lane &lane, int ref, int oth) {
		return with_thinner_bands(c, [&] { return twoview_wta_run(c, lane, &c->tv_defer[k], ref, oth, p, 0, 0); });
	};
	if ((rc = deferred_wta(0, c->main_lane(), left, right))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	progress(c, 3, "Computing cost volume for right image...");
	if (c->tv_overlap && c->tv_defer[0].queued) {
		// the first pass is queued and unverified (the dense plan): the second one beside it, from the point `go` of the
		// context's stream (before the first pass: the views and their padded planes are complete there)
		srh_context::TvSlot &T = c->tv_slot;
		HIP_TRY(hipStreamWaitEvent(T.stream, T.go, 0));
		rc = deferred_wta(1, { T.stream, &T.mem }, right, left);
		const hipError_t e = rc ? hipStreamSynchronize(T.stream) : hipEventRecord(T.done, T.stream);
		if (rc) return rc;
		if (e != hipSuccess) return fail(SRH_E_DEVICE, "second TwoView pass: %s", hipGetErrorString(e));
		HIP_TRY(hipStreamWaitEvent(c->stream, T.done, 0));            // whatever follows on the context's stream sees both maps
		// (srh_get_stats reads the context's counters and reports the last pass's, as it does without the overlap)
		HIP_TRY(hipMemcpyAsync(c->mem.cnt, T.mem.cnt, sizeof(Counters), hipMemcpyDeviceToDevice, c->stream));
	} else {
		if ((rc = deferred_wta(1, c->main_lane(), right, left))) return rc;
	}
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	srh_context::TvDefer &d0 = c->tv_defer[0], &d1 = c->tv_defer[1];
	if (d0.queued && d1.queued) {
		// both passes took the dense plan and are still unverified: queue the cross-check and the hand-over behind them, wait once
		progress(c, 5, "Detecting inconsistencies...");
		if ((rc = srh_twoview_cross_check(c, left, right, p))) return rc;
		const ViewHost &L = c->views[left], &Rv = c->views[right];
		if (left_out && !tail) HIP_TRY(hipMemcpyAsync(left_out, L.depth, (size_t)L.w*L.h*sizeof(double), hipMemcpyDeviceToHost, c->stream));
		if (right_out && !tail) HIP_TRY(hipMemcpyAsync(right_out, Rv.depth, (size_t)Rv.w*Rv.h*sizeof(double), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if (c->debug_trace)
			for (srh_context::TvDefer *d : { &d0, &d1 })
				fprintf(stderr, "[srh trace] unverified pass %d>%d: lists %d cmax %d smax %d guessed %d -> longest %d slots %d rows over %d cert_overflow %llu stands %d\n",
				        d->ref, d->oth, (int)d->lists, d->cmax, d->smax, (int)d->guessed, d->span[0], d->span[1], d->span[2],
				        (unsigned long long)d->host->cert_overflow, (int)tv_pass_stands(*d));
		if (tv_pass_stands(d0) && tv_pass_stands(d1)) {
			// a first call on guessed capacities: what the passes measured is what later calls are queued with (the tight
			// strides a verified pass would have recorded), and how the pair's lists are best evaluated
			for (srh_context::TvDefer *d : { &d0, &d1 })
				if (d->lists && d->guessed) {
					tv_learn_lists(c, d->ref, d->oth, true, d->cmax, d->smax, d->span, *d->host);
					d->guessed = false;
				}
			// (every counter of srh_stats is the LAST pass's -- right -> left -- on this path as on the verified ones and in
			// srh_get_stats, which reads the context's device counters: the second pass's were copied there above)
			c->stats.n_pixels = (int64_t)d1.host->n_pixels;
			c->stats.n_eval = (int64_t)d1.host->n_eval;
			c->stats.n_eval_device = (int64_t)d1.host->n_eval_device;
			// (the row-run certified scan counts the pixels it scanned in n_pixels: what the verified list path reports as well)
			c->stats.n_certified = d1.lists ? (d1.cert ? (int64_t)d1.host->n_pixels : 0) : (int64_t)d1.host->n_certified;
			c->stats.n_flagged = (int64_t)d1.host->n_flagged;
			c->stats.used_dense_path = d1.lists ? 0 : 1;
			c->stats.used_fused_kernel = c->last_fused ? 1 : 0;
			if (tail) {
				if (c->speckle_min_size && (rc = twoview_speckles(c, left, right, p))) return rc;
				if (c->filter_invalid && (rc = twoview_filter(c, left, right, p))) return rc;
				if (left_out && (rc = srh_view_depth_download(c, left, left_out))) return rc;
				if (right_out && (rc = srh_view_depth_download(c, right, right_out))) return rc;
			}
			progress(c, 8, "Finished!");
			return SRH_OK;
		}
		// a plan was refuted on the device (a curve off its row, a range wider than a chunk, more flagged pixels than the
		// redo covers): everything once more, each pass verified before the next step -- the maps are rewritten whole
		d0.queued = d1.queued = false;
		if ((rc = srh_twoview_wta(c, left, right, p, 0, 0))) return rc;
		if ((rc = srh_twoview_wta(c, right, left, p, 0, 0))) return rc;
	} else {
		// one pass (or none) was left unverified: settle it now, before anything reads its map
		for (int k = 0; k < 2; ++k) {
			srh_context::TvDefer &d = c->tv_defer[k];
			if (!d.queued) continue;
			HIP_TRY(hipStreamSynchronize(c->stream));
			d.queued = false;
			if (!tv_pass_stands(d) && (rc = (k == 0 ? srh_twoview_wta(c, left, right, p, 0, 0) : srh_twoview_wta(c, right, left, p, 0, 0)))) return rc;
		}
	}
	// (counters of the two passes for the statistics: an untimed recount is not worth a pass; the last pass's are reported)
	if ((rc = fetch_counters(c, c->main_lane(), c->stats.used_dense_path))) return rc;
	progress(c, 5, "Detecting inconsistencies...");
	if ((rc = srh_twoview_cross_check(c, left, right, p))) return rc;
	if (c->speckle_min_size && (rc = twoview_speckles(c, left, right, p))) return rc;
	if (c->filter_invalid && (rc = twoview_filter(c, left, right, p))) return rc;
	if (left_out && (rc = srh_view_depth_download(c, left, left_out))) return rc;
	if (right_out && (rc = srh_view_depth_download(c, right, right_out))) return rc;
	if ((rc = srh_synchronize(c))) return rc;
	progress(c, 8, "Finished!");
	return SRH_OK;
}

// The serpentine list of a view's masked-in pixels (mask.pixel == WHITE <=> byte 1; no mask: every pixel), built when the
// MultiViewStereo list path first needs it after an upload.  The device buffer keeps its capacity across uploads.
static int ensure_act(hipStream_t st, ViewHost &v) {
	if (v.act_valid) return SRH_OK;
	const int w = v.w, h = v.h;
	std::vector<uint32_t> &act = v.act_host;
	act.clear();
	act.reserve((size_t)w*h);
	v.act_row.assign((size_t)h + 1, 0u);
	for (int y = 0; y < h; ++y) {
		v.act_row[y] = (uint32_t)act.size();
		const uint8_t *mr = v.hmask.empty() ? nullptr : v.hmask.data() + (size_t)y*w;
		if (!(y & 1)) { for (int x = 0; x < w; ++x) if (!mr || mr[x] == 1) act.push_back((uint32_t)((size_t)y*w + x)); }
		else          { for (int x = w - 1; x >= 0; --x) if (!mr || mr[x] == 1) act.push_back((uint32_t)((size_t)y*w + x)); }
	}
	v.act_row[h] = (uint32_t)act.size();
	if (!act.empty()) {
		if (v.act.n < act.size()) {
			// (other streams may still read the old list: estimates of this view queued before the re-upload were settled by it)
			v.act.free();
			HIP_TRY(v.act.alloc((size_t)w*h));
		}
		HIP_TRY(hipMemcpyAsync(v.act, act.data(), act.size()*sizeof(uint32_t), hipMemcpyHostToDevice, st));
		HIP_TRY(hipStreamSynchronize(st));                  // once per upload: either slot's stream may read it next
	}
	v.act_valid = true;
	return SRH_OK;
}

// One pass of the list path of srh_mvs_initial_estimate for list capacity cmax: everything is queued on the lane's stream with
// its band buffers, nothing is waited for.  Its span[0] receives the longest list (slots), for the caller to compare with cmax.
static int mvs_list_launch(srh_context *c, const Lane &lane, int view, const int32_t *neigh, int nneigh, const srh_params *p, int y0, int y1,
                           void *peaks_dev, int cmax)
{
	int rc;
	if ((rc = ensure_act(lane.stream, c->views[view]))) return rc;
	const ViewHost &A = c->views[view];
	const int W = A.w;
	const int T = (2*p->window_radius + 1)*(2*p->window_radius + 1);
	const size_t wstride = SRH_WTILE;
	// without a refractive interface every ray of the view starts at the camera centre: the per-label
	// part of pointFromDepth is tabulated once (same operands and operations, see srh_walk.hpp)
	const bool table = !A.cam.is_refractive;
	bool neigh_pinhole = true;                                  // (certified label projections: plain pinhole neighbours only)
	for (int i = 0; i < nneigh; ++i) { const srh_camera &nc = c->views[neigh[i]].cam; if (nc.is_refractive || nc.is_distorted) neigh_pinhole = false; }
	if (table) {
		if ((rc = lane.mem->band.tnum.ensure((size_t)p->num_depth_levels))) return rc;
		Scope s(c, lane.stream, "pinhole_label_table_kernel");
		launch_pinhole_label_table(lane.stream, c->d_views, view, *p, true, lane.mem->band.tnum);
	}
	HIP_TRY(hipMemsetAsync(lane.mem->cnt, 0, sizeof(Counters), lane.stream));
	HIP_TRY(hipMemsetAsync(lane.mem->span, 0, 4*sizeof(int), lane.stream));
	const size_t per_px = (size_t)T*sizeof(double) + (size_t)nneigh*((size_t)cmax*sizeof(uint32_t) + sizeof(int32_t) + 2*sizeof(double)
	                      + (peaks_dev ? (size_t)p->top_k*2*sizeof(double) : 0));
	size_t lrows = band_budget(c) / (per_px*(size_t)W);
	if (lrows < 1) lrows = 1;
	{
		// the budget is a target, not a limit: no sliver band for a few rows over it, and bands of equal height
		const size_t rows = (size_t)(y1 - y0);
		if (rows <= lrows + lrows/4) lrows = rows;
		else { const size_t nb = (rows + lrows - 1)/lrows; lrows = (rows + nb - 1)/nb; }
	}
	const size_t units = lrows*W*(size_t)nneigh;
	// the list kernels' units: the masked-in pixels of a band, padded to whole 128-pixel blocks per link
	size_t lunits = 0;
	for (int by = y0; by < y1; by += (int)lrows) {
		const int nr = std::min((int)lrows, y1 - by);
		const size_t na = (size_t)A.act_row[by + nr] - A.act_row[by];
		lunits = std::max(lunits, ((na + 127) & ~(size_t)127)*(size_t)nneigh);
	}
	if ((rc = lane.mem->band.wbuf.ensure(wbuf_doubles(W, (int)lrows, T)))) return rc;
	if ((rc = lane.mem->band.cost.ensure(units*2 + (peaks_dev ? units*(size_t)p->top_k*2 : 0)))) return rc;   // best pairs + per-unit top-K, by pixel
	if ((rc = lane.mem->band.lcand.ensure(std::max<size_t>(lunits, 128)*(size_t)cmax))) return rc;   // wave-tiled lists
	if ((rc = lane.mem->band.lcount.ensure(std::max<size_t>(lunits, 128)))) return rc;
	const bool staged = c->mvs_staged != 0;
	if (staged) {
		int maxw; size_t words;
		mvs_staging_shape(&maxw, &words);
		const size_t waves = std::max<size_t>(lunits, 128)/64;
		if ((rc = lane.mem->band.mvs_wdesc.ensure(waves*words))) return rc;
		if ((rc = lane.mem->band.mvs_nwin.ensure(waves))) return rc;
	}
	for (int by = y0; by < y1; by += (int)lrows) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		const int nr = std::min((int)lrows, y1 - by);
		const uint32_t *act = A.act ? A.act + A.act_row[by] : nullptr;
		const int nact = (int)(A.act_row[by + nr] - A.act_row[by]);
		run_weights(c, lane, view, W, *p, by, nr, wstride);
		{ Scope s(c, lane.stream, "mvs_walk_kernel");
		  launch_mvs_walk(lane.stream, c->d_views, view, neigh, nneigh, W, *p, by, nr, table ? lane.mem->band.tnum : nullptr, lane.mem->band.lcand, cmax, lane.mem->band.lcount,
		                  lane.mem->cnt, lane.mem->span, staged ? lane.mem->band.mvs_wdesc : nullptr, staged ? lane.mem->band.mvs_nwin : nullptr, act, nact,
		                  peaks_dev != nullptr, neigh_pinhole && c->arith == 3); }
		double *const upk = peaks_dev ? lane.mem->band.cost + units*2 : nullptr;
		if (staged) {
			Scope s(c, lane.stream, "mvs_staged_cost_kernel");
			launch_mvs_staged_cost(lane.stream, c->d_views, view, neigh, nneigh, W, *p, by, nr, lane.mem->band.wbuf, wstride,
			                       lane.mem->band.lcand, cmax, lane.mem->band.lcount, lane.mem->band.cost, lane.mem->band.mvs_wdesc, lane.mem->band.mvs_nwin, lane.mem->cnt, act, nact, upk,
			                       c->arith == 3 && !peaks_dev);
		}
		{ Scope s(c, lane.stream, "mvs_list_cost_kernel");
		  launch_mvs_list_cost(lane.stream, c->d_views, view, neigh, nneigh, W, *p, by, nr, lane.mem->band.wbuf, wstride,
		                       lane.mem->band.lcand, cmax, lane.mem->band.lcount, lane.mem->band.cost, upk, peaks_dev != nullptr, staged ? lane.mem->band.mvs_nwin : nullptr, act, nact); }
		{ Scope s(c, lane.stream, "mvs_combine_kernel");
		  launch_mvs_combine(lane.stream, c->d_views, view, nneigh, W, *p, by, nr, lane.mem->band.cost, upk, (double *)peaks_dev); }
	}
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

#ifdef SRH_PROFILE_PHASES
static void mvs_print_phases(const Lane &lane) {
	Counters h;
	if (hipMemcpy(&h, lane.mem->cnt, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
	if (h.dbg_waves)
		fprintf(stderr, "[srh prof] staged MVS cost: %llu waves, %.1f windows and %.1f slots per wave; cycles per wave: life %.0f = "
		        "set-up %.0f + copies %.0f + slots %.0f (%.0f per slot) + end %.0f\n", h.dbg_waves, (double)h.dbg_cycles/h.dbg_waves,
		        (double)h.dbg_blocks/h.dbg_waves, (double)h.dbg_total_cycles/h.dbg_waves, (double)h.dbg_phase[0]/h.dbg_waves,
		        (double)h.dbg_phase[1]/h.dbg_waves, (double)h.dbg_phase[2]/h.dbg_waves,
		        h.dbg_blocks ? (double)h.dbg_phase[2]/h.dbg_blocks : 0.0, (double)h.dbg_phase[3]/h.dbg_waves);
}
#endif

// ---- two estimates in flight ------------------------------------------------------------------------------------
// The kernels of one view end in tails (the last, longest waves of the walk and cost kernels) and the call used to end
// in a host synchronisation for the list-capacity check.  The default list path now only QUEUES a view's kernels, on
// one of two side streams in turn (slot 1 with its own band buffers), so that the next view's kernels fill the
// tails of this one's; the capacity check is made when the slot is used again or when any other entry point touches
// the context (check_slot), and a view whose lists were cut is then redone.  Results are complete whenever a caller
// can observe them.

// the list path on `lane`, waited for: a pass whose lists were cut is repeated with the true maximum as the capacity
static int mvs_run_and_wait(srh_context *c, const Lane &lane, int view, const int32_t *neigh, int nneigh, const srh_params *p,
                            int y0, int y1, void *peaks_dev, int cmax)
{
	int rc;
	for (int pass = 0; pass < 3; ++pass) {
		if ((rc = mvs_list_launch(c, lane, view, neigh, nneigh, p, y0, y1, peaks_dev, cmax))) return rc;
		int maxc = 0;
		if ((rc = read_back(lane.stream, &maxc, lane.mem->span, sizeof(int)))) return rc;
#ifdef SRH_PROFILE_PHASES
		mvs_print_phases(lane);
#endif
		if (maxc <= cmax) { if (cmax > c->mvs_cmax_hint) c->mvs_cmax_hint = cmax; break; }
		cmax = (maxc + 7) & ~7;
	}
	c->mvs_last = -1;
	HIP_TRY(hipGetLastError());
	c->stats.used_dense_path = 0;
	return SRH_OK;
}

static int mvs_settle_slot(srh_context *c, int k) {
	MvsSlot &S = c->mvs_slot[k];
	if (!S.pending) return SRH_OK;
	HIP_TRY(hipStreamSynchronize(S.stream));
	S.pending = false;
	if (k == c->mvs_last && S.own_buffers)                       // srh_get_stats reads the context's counters, on its stream
		HIP_TRY(hipMemcpyAsync(c->mem.cnt, S.mem.cnt, sizeof(Counters), hipMemcpyDeviceToDevice, c->stream));
#ifdef SRH_PROFILE_PHASES
	mvs_print_phases(c->slot_lane(S));
#endif
	const int maxc = *S.h_maxc;
	if (c->debug_trace) fprintf(stderr, "[srh trace] mvs view %d settled: capacity %d, longest list %d%s\n", S.view, S.cmax, maxc, maxc <= S.cmax ? "" : " -> redone");
	if (maxc <= S.cmax) { if (S.cmax > c->mvs_cmax_hint) c->mvs_cmax_hint = S.cmax; return SRH_OK; }
	// a list was cut: redo the view, waiting for it, with the true maximum as the capacity, on the main lane (the context's
	// own scratch, which slot 0 shares: nothing may be in flight).  A refused band buffer returns straight out: the entry
	// point that settles retries (with_thinner_bands) or reports it.
	for (MvsSlot &O : c->mvs_slot) if (O.stream) HIP_TRY(hipStreamSynchronize(O.stream));
	c->mvs_cmax_hint = std::max(c->mvs_cmax_hint, (maxc + 7) & ~7);
	HIP_TRY(hipSetDevice(c->device));
	return mvs_run_and_wait(c, c->main_lane(), S.view, S.neigh, S.nneigh, &S.p, S.y0, S.y1, nullptr, c->mvs_cmax_hint);
}

static int mvs_settle_all(srh_context *c) {
	int rc;
	for (int k = 0; k < SRH_MVS_SLOTS; ++k) if ((rc = mvs_settle_slot(c, k))) return rc;
	return SRH_OK;
}

// ---- the MultiViewStereo estimate driver: argument checks, a capacity guess, and one of three runners -- queue on a slot,
// run and wait (the capacity loop), the one-thread-per-pixel kernel -- each on the lane it is handed --------

static int mvs_check_args(srh_context *c, int view, const int32_t *neigh, int nneigh, const srh_params *p, const void *peaks_dev) {
	int rc;
	if ((rc = check_slot(c, view, true, false)) || (rc = check_params(p))) return rc;
	if (nneigh < 0 || nneigh > SRH_MAX_NEIGH)
		return fail(SRH_E_UNSUPPORTED, "nneigh %d outside [0,%d] (the reference's NUM_NEIGHBOURING_VIEWS is 3)", nneigh, SRH_MAX_NEIGH);
	if (nneigh > 0 && !neigh) return fail(SRH_E_INVALID, "null neighbour list");
	if (peaks_dev && p->top_k < 1) return fail(SRH_E_INVALID, "top_k < 1");
	for (int i = 0; i < nneigh; ++i) {
		if ((rc = check_slot(c, neigh[i], true, false))) return rc;
		if (neigh[i] == view) return fail(SRH_E_INVALID, "view %d listed as its own neighbour", view);
	}
	return SRH_OK;
}

// The list capacity a view is first tried with: the longest list seen so far on this context -- or, with no hint yet, a guess
// from the geometry: the longest coarse curve over the neighbours, estimate_list_capacity (round 5 started from 2 D, which
// on the C4 rig cut every view's lists once: its first runTask took twice a later one)
static int mvs_guess_cmax(srh_context *c, int view, const int32_t *neigh, int nneigh, const srh_params *p, int y0, int y1) {
	if (c->mvs_cmax_hint > 0) return c->mvs_cmax_hint;
	const ViewHost &A = c->views[view];
	int cmax = 64;
	for (int i = 0; i < nneigh; ++i) {
		int cm = 0, sm = 0;
		const ViewHost &N = c->views[neigh[i]];
		estimate_list_capacity(A.cam, N.cam, A.w, A.h, N.w, N.h, *p, y0, y1, cm, sm, true);
		cmax = std::max(cmax, cm);
	}
	return cmax;
}

// queue the view's list path on the next slot's lane and return: the capacity check waits (mvs_settle_slot)
static int mvs_queue_on_slot(srh_context *c, int view, const int32_t *neigh, int nneigh, const srh_params *p, int y0, int y1, int cmax) {
	int rc;
	const int k = c->mvs_turn;
	c->mvs_turn = (c->mvs_turn + 1) % SRH_MVS_SLOTS;
	MvsSlot &S = c->mvs_slot[k];
	if ((rc = mvs_settle_slot(c, k))) return rc;
	cmax = std::max(cmax, c->mvs_cmax_hint);
	if (!S.stream) {
		HIP_TRY(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
		HIP_TRY(hipHostMalloc((void **)&S.h_maxc, sizeof(int)));
		*S.h_maxc = 0;
		S.own_buffers = k >= 1;
		if (S.own_buffers) {
			HIP_TRY(S.mem.cnt.alloc(1));
			HIP_TRY(S.mem.span.alloc(4));
		}
	}
	HIP_TRY(hipEventRecord(S.ev, c->stream));                     // after whatever the caller's stream holds
	HIP_TRY(hipStreamWaitEvent(S.stream, S.ev, 0));
	*S.h_maxc = 0;                                                 // (a queue that fails half-way must not leave a stale length behind)
	const Lane lane = c->slot_lane(S);
	rc = mvs_list_launch(c, lane, view, neigh, nneigh, p, y0, y1, nullptr, cmax);
	if (!rc && hipMemcpyAsync(S.h_maxc, lane.mem->span, sizeof(int), hipMemcpyDeviceToHost, lane.stream) != hipSuccess)
		rc = fail(SRH_E_DEVICE, "queueing the list-length read-back failed");
	if (rc) {
		// nothing of this view counts: drain what was queued, the slot is free again
		(void)hipStreamSynchronize(S.stream);
		S.pending = false;
		return rc;
	}
	// A caller-owned stream (srh_set_stream) keeps its contract: work the caller enqueues on it after this call
	// is ordered after the estimate.  (The context's own stream needs no such edge: every entry point settles.)
	if (c->stream != c->own_stream) {
		HIP_TRY(hipEventRecord(S.done, S.stream));
		HIP_TRY(hipStreamWaitEvent(c->stream, S.done, 0));
	}
	S.pending = true;
	S.view = view; S.nneigh = nneigh; S.y0 = y0; S.y1 = y1; S.cmax = cmax; S.p = *p;
	for (int i = 0; i < nneigh; ++i) S.neigh[i] = neigh[i];
	c->mvs_last = k;
	c->stats.used_dense_path = 0;
	return SRH_OK;
}

// other radii, no neighbours, option force_generic: the one-thread-per-pixel kernel, band by band
static int mvs_generic_run(srh_context *c, const Lane &lane, int view, const int32_t *neigh, int nneigh, const srh_params *p,
                           int y0, int y1, void *peaks_dev)
{
	int rc;
	const int W = c->views[view].w, H = c->views[view].h;
	const int T = (2*p->window_radius + 1)*(2*p->window_radius + 1);
	const int rows = band_rows(c, W, H, T);
	if ((rc = lane.mem->band.wbuf.ensure(wbuf_doubles(W, rows, T)))) return rc;
	HIP_TRY(hipMemsetAsync(lane.mem->cnt, 0, sizeof(Counters), lane.stream));
	for (int by = y0; by < y1; by += rows) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		const int nr = std::min(rows, y1 - by);
		run_weights(c, lane, view, W, *p, by, nr, SRH_WTILE);
		{ Scope s(c, lane.stream, "mvs_generic_kernel");
		  launch_mvs_generic(lane.stream, c->d_views, view, neigh, nneigh, W, *p, by, nr, lane.mem->band.wbuf, SRH_WTILE,
		                     (double *)peaks_dev, lane.mem->cnt); }
	}
	HIP_TRY(hipGetLastError());
	c->stats.used_dense_path = 0;
	return SRH_OK;
}

// default: walk kernel -> candidate lists -> cost kernel -> maximum (and merged top-K lists) over the neighbours, queued on a
// slot (option mvs_async, no peaks wanted) or waited for on the main lane.  Other radii stay on the one-thread-per-pixel kernel.
static int mvs_initial_estimate_run(srh_context *c, int view, const int32_t *neigh, int nneigh,
                                    const srh_params *p, int y0, int y1, void *peaks_dev)
{
	int rc;
	if ((rc = mvs_check_args(c, view, neigh, nneigh, p, peaks_dev))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const int W = c->views[view].w, H = c->views[view].h;
	if (y0 < 0) y0 = 0;
	if (y1 <= 0 || y1 > H) y1 = H;
	if (y1 <= y0) return SRH_OK;
	const bool lists = !c->force_generic && nneigh > 0 && p->window_radius == 2 && W < 65536 && H < 65536;
	const int cmax = lists ? mvs_guess_cmax(c, view, neigh, nneigh, p, y0, y1) : 0;
	if (lists && c->mvs_async && !peaks_dev) return mvs_queue_on_slot(c, view, neigh, nneigh, p, y0, y1, cmax);
	if ((rc = mvs_settle_all(c))) return rc;
	if (lists) return mvs_run_and_wait(c, c->main_lane(), view, neigh, nneigh, p, y0, y1, peaks_dev, cmax);
	return mvs_generic_run(c, c->main_lane(), view, neigh, nneigh, p, y0, y1, peaks_dev);
}

extern "C" int srh_mvs_initial_estimate(srh_context *c, int view, const int32_t *neigh, int nneigh,
                                        const srh_params *p, int y0, int y1, void *peaks_dev)
{
	if (!c) return fail(SRH_E_INVALID, "null context");
	return with_thinner_bands(c, [&] { return mvs_initial_estimate_run(c, view, neigh, nneigh, p, y0, y1, peaks_dev); });
}

// ---- sub-pixel depth for a view's finished map (srh_mvs_subpixel.hip): the winner search over the whole view,
// then band by band the support windows and the refine kernel.  The call's planes live in one block of the context:
// counters | neigh_xy | delta | win | cls
extern "C" int srh_mvs_view_subpixel(srh_context *c, int view, const int32_t *neigh, int nneigh, const srh_params *p,
                                     srh_mvs_subpixel_info *info, double *delta, int32_t *win, int32_t *neigh_xy, uint8_t *cls)
{
	int rc;
	if ((rc = check_slot(c, view, true)) || (rc = check_params(p))) return rc;          // (settles what "mvs_async" has in flight)
	if (nneigh < 0 || nneigh > SRH_MAX_NEIGH) return fail(SRH_E_INVALID, "nneigh %d outside [0,%d]", nneigh, SRH_MAX_NEIGH);
	if (nneigh > 0 && !neigh) return fail(SRH_E_INVALID, "null neighbour list");
	for (int i = 0; i < nneigh; ++i) {
		if ((rc = check_slot(c, neigh[i], true, false))) return rc;
		if (neigh[i] == view) return fail(SRH_E_INVALID, "view %d listed as its own neighbour", view);
	}
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &A = c->views[view];
	const int W = A.w, H = A.h;
	const size_t n = (size_t)W*H;
	const int T = (2*p->window_radius + 1)*(2*p->window_radius + 1);
	// doubles: 8 counters, 2n of neigh_xy, n of delta, 3n int32 of win (rounded up), n bytes of cls (rounded up)
	const size_t win_d = (3*n + 1)/2, cls_d = (n + 7)/8;
	if ((rc = c->mvs_subpx.ensure(SRH_MVSSUB_COUNTERS + n + 2*n + win_d + cls_d))) return rc;
	unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->mvs_subpx.p);
	int32_t *d_neigh = reinterpret_cast<int32_t *>(c->mvs_subpx + SRH_MVSSUB_COUNTERS);      // (16-byte aligned: stored as int4)
	double *d_delta = c->mvs_subpx + SRH_MVSSUB_COUNTERS + 2*n;
	int32_t *d_win = reinterpret_cast<int32_t *>(d_delta + n);
	uint8_t *d_cls = reinterpret_cast<uint8_t *>(d_delta + n + win_d);
	const Lane lane = c->main_lane();
	rc = with_thinner_bands(c, [&] {
		int rc2;
		const int rows = band_rows(c, W, H, T);
		if ((rc2 = lane.mem->band.wbuf.ensure(wbuf_doubles(W, rows, T)))) return rc2;
		HIP_TRY(hipMemsetAsync(d_cnt, 0, SRH_MVSSUB_COUNTERS*sizeof(unsigned long long), lane.stream));
		{ Scope s(c, lane.stream, "mvs_subpixel_search_kernel");
		  launch_mvs_subpixel_search(lane.stream, c->d_views, view, neigh, nneigh, W, *p, 0, H, c->mvs_subpx_search != 0, d_win, d_neigh, d_cls, d_cnt); }
		for (int by = 0; by < H; by += rows) {
			const int nr = std::min(rows, H - by);
			run_weights(c, lane, view, W, *p, by, nr, SRH_WTILE);
			Scope s(c, lane.stream, "mvs_subpixel_refine_kernel");
			launch_mvs_subpixel_refine(lane.stream, c->d_views, view, neigh, nneigh, W, *p, by, nr, lane.mem->band.wbuf, d_win, d_neigh, d_cls, d_delta, d_cnt);
		}
		HIP_TRY(hipGetLastError());
		return (int)SRH_OK;
	});
	if (rc) return rc;
	unsigned long long h_cnt[SRH_MVSSUB_COUNTERS] = { 0 };
	HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, lane.stream));
	if (delta) HIP_TRY(hipMemcpyAsync(delta, d_delta, n*sizeof(double), hipMemcpyDeviceToHost, lane.stream));
	if (neigh_xy) HIP_TRY(hipMemcpyAsync(neigh_xy, d_neigh, 4*n*sizeof(int32_t), hipMemcpyDeviceToHost, lane.stream));
	if (win) HIP_TRY(hipMemcpyAsync(win, d_win, 3*n*sizeof(int32_t), hipMemcpyDeviceToHost, lane.stream));
	if (cls) HIP_TRY(hipMemcpyAsync(cls, d_cls, n, hipMemcpyDeviceToHost, lane.stream));
	HIP_TRY(hipStreamSynchronize(lane.stream));
	if (info) {
		for (int k = 0; k < 6; ++k) info->n_class[k] = (int64_t)h_cnt[k];
		info->n_moved = (int64_t)h_cnt[6];
		info->n_fallback = (int64_t)h_cnt[7];
	}
	return SRH_OK;
}

// the view list travels once per run: MultiViewStereo::crossCheck is called per view with the same list, and a copy per
// call (from caller memory: with a host wait) put a copy, two dispatch gaps and a host round trip between the kernels
static int slots_to_device(srh_context *c, const int32_t *slots, int nviews) {
	if (c->slots_n != nviews || memcmp(c->slots_host, slots, sizeof(int32_t)*nviews) != 0) {
		c->slots_n = 0;                                             // (a failed copy must not leave a cache entry behind)
		memcpy(c->slots_host, slots, sizeof(int32_t)*nviews);
		HIP_TRY(hipMemcpyAsync(c->d_slots, c->slots_host, sizeof(int32_t)*nviews, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));                   // (the context's copy may change with the next call)
		c->slots_n = nviews;
	}
	return SRH_OK;
}

extern "C" int srh_mvs_cross_check(srh_context *c, const int32_t *slots, int nviews, int view_index,
                                   const srh_params *p)
{
	int rc;
	if (!c) return fail(SRH_E_INVALID, "null context");
	if ((rc = check_params(p))) return rc;
	if (!slots || nviews < 1 || nviews > SRH_MAX_VIEWS) return fail(SRH_E_INVALID, "bad view list");
	if (view_index < 0 || view_index >= nviews) return fail(SRH_E_INVALID, "view_index %d outside [0,%d)", view_index, nviews);
	for (int i = 0; i < nviews; ++i) if ((rc = check_slot(c, slots[i], true))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	if ((rc = slots_to_device(c, slots, nviews))) return rc;
	const ViewHost &A = c->views[slots[view_index]];
	{ Scope s(c, c->stream, "mvs_cross_check_kernel");
	  launch_mvs_cross_check(c->stream, c->d_views, c->d_slots, nviews, view_index, A.w, A.h, *p); }
	HIP_TRY(hipGetLastError());
	return SRH_OK;
}

// ------------------------------------------------------------------ depth map -> point cloud
extern "C" int srh_view_point_cloud(srh_context *c, int slot, const srh_params *p, double *xyz_out, uint8_t *rgb_out,
                                    uint8_t *valid_out, int64_t *n_points, int64_t *n_masked, int64_t *n_finite)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	// scratch: xyz (3n doubles) | rgb (3n) | valid (n) | 3 counters, in the band buffer (free between runs)
	const size_t need = 3*n + (3*n + n + 7)/8 + 4;
	if ((rc = c->mem.band.wbuf.ensure(need))) return rc;
	double *d_xyz = c->mem.band.wbuf;
	uint8_t *d_rgb = reinterpret_cast<uint8_t *>(c->mem.band.wbuf + 3*n);
	uint8_t *d_valid = d_rgb + 3*n;
	unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(c->mem.band.wbuf + need - 4);
	HIP_TRY(hipMemsetAsync(d_counts, 0, 3*sizeof(unsigned long long), c->stream));
	{ Scope s(c, c->stream, "point_cloud_kernel");
	  launch_point_cloud(c->stream, c->d_views, slot, v.w, v.h, *p, d_xyz, d_rgb, d_valid, d_counts); }
	HIP_TRY(hipGetLastError());
	unsigned long long hc[3] = { 0, 0, 0 };
	HIP_TRY(hipMemcpyAsync(hc, d_counts, sizeof(hc), hipMemcpyDeviceToHost, c->stream));
	if (xyz_out) HIP_TRY(hipMemcpyAsync(xyz_out, d_xyz, 3*n*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (rgb_out) HIP_TRY(hipMemcpyAsync(rgb_out, d_rgb, 3*n, hipMemcpyDeviceToHost, c->stream));
	if (valid_out) HIP_TRY(hipMemcpyAsync(valid_out, d_valid, n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (n_points) *n_points = (int64_t)hc[0];
	if (n_masked) *n_masked = (int64_t)hc[1];
	if (n_finite) *n_finite = (int64_t)hc[2];
	return SRH_OK;
}

// ------------------------------------------------------------------ depth-map fusion (srh_fuse.hip)
extern "C" void srh_fuse_params_defaults(srh_fuse_params *f) {
	if (!f) return;
	f->dist_threshold = 0; f->normal_depth_gap = 0; f->min_views = 2; f->flags = 0;
}

// the arrays of a cloud of `cap` points in one block of doubles: xyz | normals | src | rgb | nviews | flags
static size_t fuse_cloud_doubles(size_t cap) { return 7*cap + (5*cap + 7)/8; }
static FuseCloud fuse_cloud_carve(double *base, size_t cap) {
	FuseCloud f;
	f.xyz = base; f.nrm = base + 3*cap;
	f.src = reinterpret_cast<int32_t *>(base + 6*cap);
	f.rgb = reinterpret_cast<uint8_t *>(base + 7*cap);
	f.nviews = f.rgb + 3*cap; f.flags = f.nviews + cap;
	return f;
}

extern "C" int srh_mvs_fuse(srh_context *c, const int32_t *slots, int nviews, const srh_params *p, const srh_fuse_params *fp,
                            srh_fuse_info *info)
{
	int rc;
	if (!c) return fail(SRH_E_INVALID, "null context");
	if ((rc = check_params(p))) return rc;
	if (!slots || nviews < 1 || nviews > SRH_MAX_VIEWS) return fail(SRH_E_INVALID, "bad view list");
	srh_fuse_params f;
	srh_fuse_params_defaults(&f);
	if (fp) f = *fp;
	if (f.min_views < 1) return fail(SRH_E_INVALID, "min_views %d < 1", f.min_views);
	for (int i = 0; i < nviews; ++i) {
		if ((rc = check_slot(c, slots[i], true))) return rc;
		for (int k = 0; k < i; ++k) if (slots[k] == slots[i]) return fail(SRH_E_INVALID, "view slot %d listed twice", slots[i]);
	}
	HIP_TRY(hipSetDevice(c->device));
	c->fuse_valid = false; c->fuse_n = 0;
	if ((rc = slots_to_device(c, slots, nviews))) return rc;
	const double thr = f.dist_threshold > 0 ? f.dist_threshold : p->cross_check_threshold;
	const double gap = f.normal_depth_gap > 0 ? f.normal_depth_gap : 2*(p->max_depth - p->min_depth)/(p->num_depth_levels - 1);

	// scratch, in doubles: point maps (3T) | staging xyz, normals (3M each) | block offsets (NB) | counters (8) | point-cloud
	// counters (4) | view table (3 per view) | block counts (NB u32) | bytes: has-a-point (T), claimed (T), emit (M), staging
	// rgb (3M), nviews (M), flags (M) -- T = pixels of all views, M = of the largest, NB = its blocks
	size_t T = 0, M = 0;
	for (int i = 0; i < nviews; ++i) { const ViewHost &v = c->views[slots[i]]; const size_t n = (size_t)v.w*v.h; T += n; M = std::max(M, n); }
	const size_t NB = (M + SRH_FUSE_BLOCK - 1)/SRH_FUSE_BLOCK;
	static_assert(sizeof(FuseViewDev) == 3*sizeof(double), "view table entries are three pointers");
	const size_t need = 3*T + 6*M + NB + 8 + 4 + 3*(size_t)nviews + (NB + 1)/2 + (2*T + 6*M + 7)/8;
	if ((rc = c->fuse_scratch.ensure(need))) return rc;
	double *q = c->fuse_scratch;
	double *d_pts = q; q += 3*T;
	FuseCloud stage = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	stage.xyz = q; q += 3*M;
	stage.nrm = q; q += 3*M;
	unsigned long long *d_offs = reinterpret_cast<unsigned long long *>(q); q += NB;
	unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(q); q += 8;
	unsigned long long *d_pc = reinterpret_cast<unsigned long long *>(q); q += 4;
	FuseViewDev *d_fv = reinterpret_cast<FuseViewDev *>(q); q += 3*(size_t)nviews;
	uint32_t *d_bcount = reinterpret_cast<uint32_t *>(q); q += (NB + 1)/2;
	uint8_t *d_valid = reinterpret_cast<uint8_t *>(q), *d_claimed = d_valid + T, *d_emit = d_claimed + T;
	stage.rgb = d_emit + M; stage.nviews = stage.rgb + 3*M; stage.flags = stage.nviews + M;

	std::vector<FuseViewDev> fv((size_t)nviews);
	{
		size_t off = 0;
		for (int i = 0; i < nviews; ++i) {
			const ViewHost &v = c->views[slots[i]];
			fv[i].pts = d_pts + 3*off; fv[i].valid = d_valid + off; fv[i].claimed = d_claimed + off;
			off += (size_t)v.w*v.h;
		}
	}
	HIP_TRY(hipMemcpyAsync(d_fv, fv.data(), sizeof(FuseViewDev)*nviews, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemsetAsync(d_counters, 0, 12*sizeof(unsigned long long), c->stream));   // the counters and the point-cloud counters
	HIP_TRY(hipMemsetAsync(d_claimed, 0, T, c->stream));
	// stage 0: every view's point map, by the kernel of srh_view_point_cloud
	for (int i = 0; i < nviews; ++i) {
		const ViewHost &v = c->views[slots[i]];
		Scope s(c, c->stream, "point_cloud_kernel");
		launch_point_cloud(c->stream, c->d_views, slots[i], v.w, v.h, *p, const_cast<double *>(fv[i].pts), nullptr,
		                   const_cast<uint8_t *>(fv[i].valid), d_pc);
	}
	HIP_TRY(hipGetLastError());
	unsigned long long pc[3] = { 0, 0, 0 };
	HIP_TRY(hipMemcpyAsync(pc, d_pc, sizeof(pc), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	// the result: room for every pixel with a point (what min_views = 1 and disjoint views would emit)
	const size_t cap = (size_t)pc[0];
	FuseCloud out = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	if (cap) {
		if ((rc = c->fuse_result.ensure(fuse_cloud_doubles(cap)))) return rc;
		out = fuse_cloud_carve(c->fuse_result, cap);
	}
	// stage 1: the list's entries in order on the one stream
	for (int i = 0; i < nviews; ++i) {
		if (cancelled(c)) {
			(void)hipStreamSynchronize(c->stream);
			c->fuse_scratch.release();
			return fail(SRH_E_CANCELLED, "cancelled");
		}
		const ViewHost &v = c->views[slots[i]];
		const size_t n = (size_t)v.w*v.h;
		{ Scope s(c, c->stream, "fuse_view_kernel");
		  launch_fuse_view(c->stream, c->d_views, c->d_slots, nviews, i, v.w, v.h, *p, thr, gap, f.min_views, d_fv, d_emit, stage,
		                   d_bcount, d_counters); }
		{ Scope s(c, c->stream, "fuse_scan_kernel");
		  launch_fuse_scan(c->stream, d_bcount, (int)((n + SRH_FUSE_BLOCK - 1)/SRH_FUSE_BLOCK), d_offs, d_counters); }
		{ Scope s(c, c->stream, "fuse_scatter_kernel");
		  launch_fuse_scatter(c->stream, i, n, d_emit, stage, d_offs, out, cap); }
	}
	HIP_TRY(hipGetLastError());
	unsigned long long hc[5] = { 0, 0, 0, 0, 0 };
	HIP_TRY(hipMemcpyAsync(hc, d_counters, sizeof(hc), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->fuse_scratch.release();                                      // (idle: the stream has just been waited for)
	if (hc[4] != hc[0] || hc[0] > cap) return fail(SRH_E_DEVICE, "fusion: %llu points counted, %llu placed, room for %zu", hc[0], hc[4], cap);
	c->fuse_out = out; c->fuse_n = (int64_t)hc[0]; c->fuse_valid = true;
	if (info) {
		info->n_points = (int64_t)hc[0]; info->n_candidates = (int64_t)pc[0]; info->n_claimed = (int64_t)hc[1];
		info->n_unsupported = (int64_t)hc[2]; info->n_normals = (int64_t)hc[3];
	}
	return SRH_OK;
}

static int fuse_result_check(srh_context *c) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (!c->fuse_valid) return fail(SRH_E_INVALID, "the context holds no fused cloud (no srh_mvs_fuse yet, or the last one failed)");
	return SRH_OK;
}

extern "C" int srh_mvs_fused_count(srh_context *c, int64_t *n) {
	int rc;
	if ((rc = fuse_result_check(c))) return rc;
	if (!n) return fail(SRH_E_INVALID, "null n");
	*n = c->fuse_n;
	return SRH_OK;
}

extern "C" int srh_mvs_fused_download(srh_context *c, int64_t first, int64_t count, double *xyz, double *normals, uint8_t *rgb,
                                      uint8_t *nviews, uint8_t *flags, int32_t *src)
{
	int rc;
	if ((rc = fuse_result_check(c))) return rc;
	if (first < 0 || count < 0 || first > c->fuse_n || count > c->fuse_n - first)
		return fail(SRH_E_INVALID, "points [%lld, %lld + %lld) outside [0, %lld]", (long long)first, (long long)first, (long long)count, (long long)c->fuse_n);
	if (count == 0) return SRH_OK;
	HIP_TRY(hipSetDevice(c->device));
	const FuseCloud &o = c->fuse_out;
	const size_t a = (size_t)first, k = (size_t)count;
	if (xyz)     HIP_TRY(hipMemcpyAsync(xyz, o.xyz + 3*a, 3*k*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (normals) HIP_TRY(hipMemcpyAsync(normals, o.nrm + 3*a, 3*k*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (rgb)     HIP_TRY(hipMemcpyAsync(rgb, o.rgb + 3*a, 3*k, hipMemcpyDeviceToHost, c->stream));
	if (nviews)  HIP_TRY(hipMemcpyAsync(nviews, o.nviews + a, k, hipMemcpyDeviceToHost, c->stream));
	if (flags)   HIP_TRY(hipMemcpyAsync(flags, o.flags + a, k, hipMemcpyDeviceToHost, c->stream));
	if (src)     HIP_TRY(hipMemcpyAsync(src, o.src + 2*a, 2*k*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

extern "C" int srh_mvs_fused_device(srh_context *c, void **xyz, void **normals, void **rgb, void **nviews, void **flags, void **src) {
	int rc;
	if ((rc = fuse_result_check(c))) return rc;
	const bool any = c->fuse_n > 0;
	const FuseCloud &o = c->fuse_out;
	if (xyz) *xyz = any ? o.xyz : nullptr;
	if (normals) *normals = any ? o.nrm : nullptr;
	if (rgb) *rgb = any ? o.rgb : nullptr;
	if (nviews) *nviews = any ? o.nviews : nullptr;
	if (flags) *flags = any ? o.flags : nullptr;
	if (src) *src = any ? (void *)o.src : nullptr;
	return SRH_OK;
}

// ------------------------------------------------------------------ hole filling (srh_filter.hip)
// One map: G = the gap-filled map (or a copy of D) in the band buffer, then the holes of D listed and NaN written where
// the mask is not WHITE, then the median of every listed hole from G into D.  emit7: progress step 7 before the median
// (srh_twoview_compute, first map).
static int filter_view(srh_context *c, int slot, const srh_params *p, int flags, int gap, srh_filter_info *info, bool emit7)
{
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	const bool gaps = (flags & SRH_FILTER_GAPS) != 0, median = (flags & SRH_FILTER_MEDIAN) != 0;
	// scratch: G (n doubles) | hole list (n u32) | 4 counters, in the band buffer (free between runs)
	const size_t need = n + (n + 1)/2 + 4;
	int rc;
	if ((rc = c->mem.band.wbuf.ensure(need))) return rc;
	double *G = c->mem.band.wbuf;
	uint32_t *holes = reinterpret_cast<uint32_t *>(c->mem.band.wbuf + n);
	unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->mem.band.wbuf + need - 4);
	HIP_TRY(hipMemsetAsync(d_cnt, 0, 4*sizeof(unsigned long long), c->stream));
	if (gaps) {
		Scope s(c, c->stream, "filter_gap_kernel");
		launch_filter_gaps(c->stream, v.depth, G, v.w, v.h, gap, d_cnt);
	} else if (median) HIP_TRY(hipMemcpyAsync(G, v.depth, n*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(hipGetLastError());
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	{ Scope s(c, c->stream, "filter_holes_kernel");
	  launch_filter_holes(c->stream, v.mask, v.depth, v.w, v.h, median, holes, d_cnt); }
	HIP_TRY(hipGetLastError());
	unsigned long long hc[4] = { 0, 0, 0, 0 };
	HIP_TRY(hipMemcpyAsync(hc, d_cnt, sizeof(hc), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (median) {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		if (emit7) progress(c, 7, "Filtering invalid pixels...");
		// (option "filter_replay": the replay is the kernel's only selection today -- every hole takes it either way)
		{ Scope s(c, c->stream, "filter_median_kernel");
		  launch_filter_median(c->stream, c->d_views, slot, *p, G, holes, (int)hc[0], v.depth, d_cnt); }
		HIP_TRY(hipGetLastError());
	} else if (gaps) HIP_TRY(hipMemcpyAsync(v.depth, G, n*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(hc, d_cnt, sizeof(hc), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (info) {
		info->holes = (int64_t)hc[0];
		info->gap_filled = (int64_t)hc[1];
		info->median_filled = (int64_t)hc[2];
		info->replayed = (int64_t)hc[3];
	}
	return SRH_OK;
}

static int check_filter(srh_context *c, int slot, const srh_params *p, int flags)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	if (flags < 0 || flags > (SRH_FILTER_GAPS | SRH_FILTER_MEDIAN)) return fail(SRH_E_INVALID, "filter flags %d unknown", flags);
	if ((flags & SRH_FILTER_MEDIAN) && p->window_radius > 5)
		return fail(SRH_E_UNSUPPORTED, "weighted median: window_radius %d > 5", p->window_radius);
	// filter_median_kernel skips the taps outside the image; the reference reads depths there and keeps such a tap when
	// its window weight exp(-geodesic_init/geodesic_sigma) is > 1e-10 (srh_filter.hip): the skip is its result only below
	if ((flags & SRH_FILTER_MEDIAN) && p->weight_kind == SRH_WEIGHT_GEODESIC &&
	    !(p->geodesic_sigma > 0 && exp(-p->geodesic_init/p->geodesic_sigma) <= 1e-10))
		return fail(SRH_E_UNSUPPORTED, "weighted median: geodesic_init %g, geodesic_sigma %g give the taps outside the image a weight above 1e-10",
		            p->geodesic_init, p->geodesic_sigma);
	if ((size_t)c->views[slot].w*c->views[slot].h >= ((size_t)1 << 31))
		return fail(SRH_E_UNSUPPORTED, "hole filling: view of %d x %d pixels", c->views[slot].w, c->views[slot].h);
	return SRH_OK;
}

extern "C" int srh_view_filter_invalid(srh_context *c, int slot, const srh_params *p, int flags, int gap_width,
                                       srh_filter_info *info)
{
	int rc;
	if ((rc = check_filter(c, slot, p, flags))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	if (info) *info = srh_filter_info();
	return filter_view(c, slot, p, flags, gap_width, info, false);
}

// srh_twoview_compute's tail with option "filter_invalid" (filterInvalidPixels at the #if 0 call site, :200-223):
// both maps, progress 6, and 7 before the first median.  (The reference's right-map loop tests left.width() (:748):
// moot, TwoView views are equal-sized -- each map here is filled over its own width.)
static int twoview_filter(srh_context *c, int left, int right, const srh_params *p)
{
	int rc;
	const int flags = c->filter_invalid;
	if ((rc = check_filter(c, left, p, flags)) || (rc = check_filter(c, right, p, flags))) return rc;
	progress(c, 6, "Filling invalid pixels...");
	if ((rc = filter_view(c, left, p, flags, c->filter_gap_width, nullptr, true))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	return filter_view(c, right, p, flags, c->filter_gap_width, nullptr, false);
}

// ------------------------------------------------------------------ speckle filter (srh_speckle.hip)
extern "C" void srh_speckle_params_defaults(srh_speckle_params *s)
{
	if (!s) return;
	s->max_diff = 0; s->min_size = 0; s->flags = 0;
}

// what needs no device: the slot, the parameters, and the max_diff the call runs with
static int check_speckles(srh_context *c, int slot, const srh_params *p, const srh_speckle_params &s, double *max_diff)
{
	int rc;
	if ((rc = check_slot(c, slot, true))) return rc;
	if (!p) return fail(SRH_E_INVALID, "null params");
	if (s.min_size < 0) return fail(SRH_E_INVALID, "speckle filter: min_size %d < 0", s.min_size);
	if (s.flags & ~SRH_SPECKLE_TO_NAN) return fail(SRH_E_INVALID, "speckle filter: flags %d unknown", s.flags);
	if (!std::isfinite(s.max_diff)) return fail(SRH_E_INVALID, "speckle filter: max_diff is not finite");
	*max_diff = s.max_diff;
	if (!(s.max_diff > 0)) {
		if (p->num_depth_levels < 2) return fail(SRH_E_INVALID, "speckle filter: the default max_diff needs num_depth_levels >= 2, not %d", p->num_depth_levels);
		*max_diff = cc::depth_steps(p->min_depth, p->max_depth, p->num_depth_levels, 2.0);
		if (!std::isfinite(*max_diff)) return fail(SRH_E_INVALID, "speckle filter: min_depth %g, max_depth %g give no finite depth step", p->min_depth, p->max_depth);
	}
	if ((size_t)c->views[slot].w*c->views[slot].h >= ((size_t)1 << 31))
		return fail(SRH_E_UNSUPPORTED, "speckle filter: view of %d x %d pixels", c->views[slot].w, c->views[slot].h);
	return SRH_OK;
}

// One map.  Scratch in the band buffer (free between runs): the label planes A | B (n int32 each) | 5 counters.
static int speckle_view(srh_context *c, int slot, double max_diff, int min_size, bool to_nan, srh_speckle_info *info, int32_t *labels_out)
{
	const ViewHost &v = c->views[slot];
	const size_t n = (size_t)v.w*v.h;
	int rc;
	if ((rc = c->mem.band.wbuf.ensure(n + 5))) return rc;
	int32_t *A = reinterpret_cast<int32_t *>((double *)c->mem.band.wbuf), *B = A + n;
	unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->mem.band.wbuf + n);
	HIP_TRY(hipMemsetAsync(d_cnt, 0, 5*sizeof(unsigned long long), c->stream));
	{ Scope s(c, c->stream, "speckle_tile_kernel");
	  launch_speckle_tiles(c->stream, v.mask, v.depth, v.w, v.h, max_diff, A); }
	HIP_TRY(hipGetLastError());
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	{ Scope s(c, c->stream, "speckle_merge_kernel");
	  launch_speckle_merge(c->stream, v.depth, v.w, v.h, max_diff, A); }
	HIP_TRY(hipGetLastError());
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	{ Scope s(c, c->stream, "speckle_flatten_kernel");
	  launch_speckle_flatten(c->stream, A, n, B); }
	HIP_TRY(hipGetLastError());
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	HIP_TRY(hipMemsetAsync(A, 0, n*sizeof(int32_t), c->stream));       // A: the sizes, at the components' labels
	{ Scope s(c, c->stream, "speckle_count_kernel");
	  launch_speckle_count(c->stream, B, n, A); }
	HIP_TRY(hipGetLastError());
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	{ Scope s(c, c->stream, "speckle_apply_kernel");
	  launch_speckle_apply(c->stream, B, A, n, min_size, to_nan ? (double)NAN : (double)INFINITY, v.depth, d_cnt); }
	HIP_TRY(hipGetLastError());
	unsigned long long hc[5] = { 0, 0, 0, 0, 0 };
	if (info) HIP_TRY(hipMemcpyAsync(hc, d_cnt, sizeof(hc), hipMemcpyDeviceToHost, c->stream));
	if (labels_out) HIP_TRY(hipMemcpyAsync(labels_out, B, n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (info) {
		info->valid = (int64_t)hc[0];
		info->components = (int64_t)hc[1];
		info->removed_components = (int64_t)hc[2];
		info->removed_pixels = (int64_t)hc[3];
		info->largest = (int64_t)hc[4];
	}
	return SRH_OK;
}

extern "C" int srh_view_filter_speckles(srh_context *c, int slot, const srh_params *p, const srh_speckle_params *s,
                                        srh_speckle_info *info, int32_t *labels_out)
{
	int rc;
	srh_speckle_params sp;
	srh_speckle_params_defaults(&sp);
	if (s) sp = *s;
	double max_diff = 0;
	if ((rc = check_speckles(c, slot, p, sp, &max_diff))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	if (info) *info = srh_speckle_info();
	return speckle_view(c, slot, max_diff, sp.min_size, (sp.flags & SRH_SPECKLE_TO_NAN) != 0, info, labels_out);
}

// srh_twoview_compute*'s stage under option "speckle_min_size": both maps, reject value +INF, behind the cross-check and
// before the hole filling; its own stage text at the cross-check's progress step
static int twoview_speckle_params(srh_context *c, const srh_params *p, srh_speckle_params *s)
{
	s->min_size = c->speckle_min_size; s->flags = 0;
	s->max_diff = cc::depth_steps(p->min_depth, p->max_depth, p->num_depth_levels, (double)c->speckle_diff_steps);
	if (!(s->max_diff > 0)) return fail(SRH_E_INVALID, "speckle_diff_steps %d of depth range [%g, %g] give no positive max_diff", c->speckle_diff_steps, p->min_depth, p->max_depth);
	return SRH_OK;
}

static int check_twoview_speckles(srh_context *c, int left, int right, const srh_params *p)
{
	int rc;
	srh_speckle_params s;
	double max_diff;
	if ((rc = check_params(p)) || (rc = twoview_speckle_params(c, p, &s))) return rc;
	if ((rc = check_speckles(c, left, p, s, &max_diff)) || (rc = check_speckles(c, right, p, s, &max_diff))) return rc;
	return SRH_OK;
}

static int twoview_speckles(srh_context *c, int left, int right, const srh_params *p)
{
	int rc;
	srh_speckle_params s;
	double max_diff = 0;
	if ((rc = twoview_speckle_params(c, p, &s))) return rc;
	if ((rc = check_speckles(c, left, p, s, &max_diff)) || (rc = check_speckles(c, right, p, s, &max_diff))) return rc;
	progress(c, 5, "Removing speckles...");
	if ((rc = speckle_view(c, left, max_diff, s.min_size, false, nullptr, nullptr))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	return speckle_view(c, right, max_diff, s.min_size, false, nullptr, nullptr);
}

// ------------------------------------------------------------------ rectification (srh_rectify.hpp / .hip)
extern "C" void srh_rectify_params_defaults(srh_rectify_params *r)
{
	if (!r) return;
	r->focal = 0; r->cx_a = r->cx_b = r->cy = __builtin_nan("");
	r->out_w = r->out_h = 0; r->flags = r->reserved = 0;
}

extern "C" int srh_twoview_row_aligned(const srh_camera *a, const srh_camera *b, double *fx_bx)
{
	if (!a || !b) return 0;
	double f = 0;
	const bool yes = rig_is_row_aligned(*a, *b, &f);
	if (yes && fx_bx) *fx_bx = f;
	return yes ? 1 : 0;
}

extern "C" int srh_rectify_cameras(const srh_camera *a, const srh_camera *b, int w, int h, double image_scale,
                                   const srh_rectify_params *r, srh_camera *ra, srh_camera *rb)
{
	if (!a || !b || !ra || !rb) return fail(SRH_E_INVALID, "null argument");
	srh_rectify_params rp;
	srh_rectify_params_defaults(&rp);
	if (r) rp = *r;
	rect::Geometry g;
	const char *why = "";
	int rc = rect::geometry(*a, *b, w, h, image_scale, rp, g, &why);
	if (rc) return fail(rc, "rectification: %s", why);
	srh_camera ca, cb;
	if ((rc = srh_camera_from_krt(g.Ka, g.Rn, g.ta, nullptr, nullptr, 0.0, 1.0, &ca))) return rc;
	if ((rc = srh_camera_from_krt(g.Kb, g.Rn, g.tb, nullptr, nullptr, 0.0, 1.0, &cb))) return rc;
	*ra = ca; *rb = cb;
	return SRH_OK;
}

extern "C" int srh_view_rectify_map(srh_context *c, int src_slot, const srh_camera *rect_cam, int out_w, int out_h,
                                    double image_scale, double *uv_out)
{
	int rc;
	if ((rc = check_slot(c, src_slot, true))) return rc;
	if (!rect_cam || !uv_out) return fail(SRH_E_INVALID, "null argument");
	if (out_w <= 0 || out_h <= 0 || out_w > SRH_MAX_VIEW_DIM || out_h > SRH_MAX_VIEW_DIM) return fail(SRH_E_INVALID, "bad output size %dx%d", out_w, out_h);
	if (!(image_scale > 0) || !std::isfinite(image_scale)) return fail(SRH_E_INVALID, "image_scale must be > 0");
	if (c->views[src_slot].cam.is_refractive || rect_cam->is_refractive) return fail(SRH_E_UNSUPPORTED, "rectification: a refractive camera");
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)out_w*out_h;
	DevBuf<double> uv;
	hipError_t e = uv.alloc(2*n);
	if (e == hipSuccess) {
		Scope s(c, c->stream, "rectify_warp_kernel");
		launch_rectify_warp(c->stream, c->d_views, src_slot, *rect_cam, out_w, out_h, image_scale, uv, nullptr, nullptr);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(uv_out, uv, 2*n*sizeof(double), hipMemcpyDeviceToHost, c->stream);
	const hipError_t es = hipStreamSynchronize(c->stream);
	uv.release();
	if (e == hipSuccess) e = es;
	if (e != hipSuccess) return fail(SRH_E_DEVICE, "rectification map: %s", hipGetErrorString(e));
	return SRH_OK;
}

extern "C" int srh_twoview_rectify(srh_context *c, int src_a, int src_b, int dst_a, int dst_b, const srh_params *p,
                                   const srh_rectify_params *r, srh_rectify_info *info)
{
	int rc;
	if ((rc = check_slot(c, src_a, true)) || (rc = check_slot(c, src_b, true)) || (rc = check_slot(c, dst_a, false)) ||
	    (rc = check_slot(c, dst_b, false)) || (rc = check_params(p))) return rc;
	if (src_a == src_b || dst_a == dst_b) return fail(SRH_E_INVALID, "rectification: the two sources (and the two destinations) are different slots");
	// every refusal comes before a slot is touched
	const srh_camera old_a = c->views[src_a].cam, old_b = c->views[src_b].cam;   // (copies: a source may be a destination)
	const int aw = c->views[src_a].w, ah = c->views[src_a].h;
	srh_rectify_params rp;
	srh_rectify_params_defaults(&rp);
	if (r) rp = *r;
	srh_camera cam[2];
	if ((rc = srh_rectify_cameras(&old_a, &old_b, aw, ah, p->image_scale, &rp, &cam[0], &cam[1]))) return rc;
	const int ow = rp.out_w ? rp.out_w : aw, oh = rp.out_h ? rp.out_h : ah;
	const size_t n = (size_t)ow*oh;
	HIP_TRY(hipSetDevice(c->device));
	// both warps are queued (and finished) before either destination is installed: a destination may be a source
	DevBuf<uint32_t> img[2];
	DevBuf<uint8_t> msk[2];
	std::vector<uint8_t> hmask[2];
	const int src[2] = { src_a, src_b }, dst[2] = { dst_a, dst_b };
	auto run = [&]() -> int {
		for (int k = 0; k < 2; ++k) {
			HIP_TRY(img[k].alloc(n));
			HIP_TRY(msk[k].alloc(n));
			hmask[k].resize(n);
		}
		for (int k = 0; k < 2; ++k) {
			{ Scope s(c, c->stream, "rectify_warp_kernel");
			  launch_rectify_warp(c->stream, c->d_views, src[k], cam[k], ow, oh, p->image_scale, nullptr, img[k], msk[k]); }
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(hmask[k].data(), msk[k], n, hipMemcpyDeviceToHost, c->stream));
		}
		HIP_TRY(hipStreamSynchronize(c->stream));
		for (int k = 0; k < 2; ++k) {
			const int r2 = view_install(c, dst[k], ow, oh, img[k], msk[k], hmask[k].data(), hipMemcpyDeviceToDevice, &cam[k]);
			if (r2) return r2;
		}
		return SRH_OK;
	};
	rc = run();
	(void)hipStreamSynchronize(c->stream);
	for (int k = 0; k < 2; ++k) { img[k].release(); msk[k].release(); }
	if (rc) return rc;
	if (info) {
		info->angle_a = rect::axis_angle(old_a, cam[0]);
		info->angle_b = rect::axis_angle(old_b, cam[1]);
		info->fx_bx = 0;
		(void)rig_is_row_aligned(cam[0], cam[1], &info->fx_bx);
		int64_t wc[2] = { 0, 0 };
		for (int k = 0; k < 2; ++k) for (size_t i = 0; i < n; ++i) wc[k] += hmask[k][i] == 1;
		info->white_a = wc[0]; info->white_b = wc[1];
	}
	return SRH_OK;
}

extern "C" int srh_view_depth_unrectify(srh_context *c, int rect_slot, int dst_slot, const srh_params *p, int32_t *src_index_out)
{
	int rc;
	if ((rc = check_slot(c, rect_slot, true)) || (rc = check_slot(c, dst_slot, true)) || (rc = check_params(p))) return rc;
	if (rect_slot == dst_slot) return fail(SRH_E_INVALID, "unrectify: the rectified view and the destination are the same slot");
	ViewHost &D = c->views[dst_slot];
	const ViewHost &R = c->views[rect_slot];
	if (D.cam.is_refractive || R.cam.is_refractive) return fail(SRH_E_UNSUPPORTED, "unrectify: a refractive camera");
	const Vec3 dc = load3(D.cam.C) - load3(R.cam.C);
	if (!(norm(dc) <= 1e-9*(1.0 + norm(load3(D.cam.C)))))
		return fail(SRH_E_INVALID, "unrectify: the cameras of slots %d and %d do not share a centre (distance %g)", rect_slot, dst_slot, norm(dc));
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)D.w*D.h;
	DevBuf<int32_t> index;
	hipError_t e = hipSuccess;
	if (src_index_out) e = index.alloc(n);
	if (e == hipSuccess) {
		Scope s(c, c->stream, "unrectify_kernel");
		launch_unrectify(c->stream, c->d_views, rect_slot, dst_slot, D.w, D.h, p->image_scale, index);
		e = hipGetLastError();
	}
	if (e == hipSuccess && src_index_out) e = hipMemcpyAsync(src_index_out, index, n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
	const hipError_t es = hipStreamSynchronize(c->stream);
	index.release();
	if (e == hipSuccess) e = es;
	if (e != hipSuccess) return fail(SRH_E_DEVICE, "unrectify: %s", hipGetErrorString(e));
	D.wta_flags = 0;                                             // the map no longer comes from a WTA pass of this view
	return SRH_OK;
}

// ------------------------------------------------------------------ epipolar curves on request
extern "C" int srh_epipolar_curves(srh_context *c, int ref, int oth, const srh_params *p, int mvs,
                                   int nq, const int32_t *xy, int32_t *out_xy, int max_pts, int32_t *counts)
{
	int rc;
	if ((rc = check_slot(c, ref, true)) || (rc = check_slot(c, oth, true)) || (rc = check_params(p))) return rc;
	if (ref == oth) return fail(SRH_E_INVALID, "ref and other view are the same slot");
	if (nq < 0 || max_pts < 0 || (nq > 0 && (!xy || !counts)) || (nq > 0 && max_pts > 0 && !out_xy))
		return fail(SRH_E_INVALID, "bad query buffers");
	if (nq == 0) return SRH_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf<int32_t> d_xy, d_out, d_n;
	const size_t out_bytes = (size_t)nq*2*(size_t)max_pts*sizeof(int32_t);
	hipError_t e = d_xy.alloc((size_t)nq*2);
	if (e == hipSuccess) e = d_n.alloc(nq);
	if (e == hipSuccess && out_bytes) e = d_out.alloc((size_t)nq*2*(size_t)max_pts);
	if (e == hipSuccess) e = hipMemcpyAsync(d_xy, xy, (size_t)nq*2*sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) {
		Scope s(c, c->stream, "epipolar_curves_kernel");
		launch_epipolar_curves(c->stream, c->d_views, ref, oth, *p, mvs ? 1 : 0, nq, d_xy, d_out, max_pts, d_n);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(counts, d_n, (size_t)nq*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess && out_bytes) e = hipMemcpyAsync(out_xy, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	else (void)hipStreamSynchronize(c->stream);
	d_xy.free(); d_n.free(); d_out.free();
	if (e != hipSuccess) return fail(SRH_E_DEVICE, "epipolar curves: %s", hipGetErrorString(e));
	return SRH_OK;
}

// ------------------------------------------------------------------ MultiViewStereo, MRF branch
extern "C" void srh_mrf_params_defaults(srh_mrf_params *m)
{
	if (!m) return;
	m->beta = 1; m->lambda = 1; m->phi_u = 0.5; m->psi_u = 0.002;     // multiviewstereo.cpp:98-101
	m->max_iters = 50; m->min_energy_drop = 5;                       // :631, :641
}

// The label-volume stages (LabelStage; the four sections from here on) check a run's device memory before anything is
// queued: `n` doubles in each buffer.  What is missing must fit the free memory + the pool + the outgrown buffers (released
// first); under option mem_limit_mb the whole need must fit the pretended device.  refuse(need, avail), in bytes, words the refusal.
struct StageWant { DevBuf<double> *buf; size_t n; };
template <class Refuse>
static int stage_reserve(srh_context *c, const StageWant *wants, int nwants, Refuse refuse)
{
	size_t need = 0, missing = 0, held = 0;
	for (int i = 0; i < nwants; ++i) {
		need += wants[i].n*sizeof(double);
		if (wants[i].buf->n < wants[i].n) { missing += wants[i].n*sizeof(double); held += wants[i].buf->bytes(); }
	}
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
		size_t avail = free_b + pool_bytes_on(c->device) + held;
		size_t want = missing;
		if (c->mem_limit) { want = need; if (avail > c->mem_limit) avail = c->mem_limit; }
		if (want > avail) return refuse(need, avail);
	} else (void)hipGetLastError();
	for (int i = 0; i < nwants; ++i) if (const int rc = wants[i].buf->ensure(wants[i].n)) return rc;
	return SRH_OK;
}

// One view's run of a MultiViewStereo optimiser: the K peaks of the w x h view in `slot`, on stream `st` in `scratch`: the
// context's for a one-view entry point, a stream and a scratch per view (mvs_view_runs) for the views side by side
struct MvsRun { int slot, w, h, K; hipStream_t st; DevBuf<double> *scratch; const double *peaks; };

// The runs of the listed views: run i on c->mrf_stream[i], behind what the context's stream holds (the peaks were written
// there), on the view's own scratch, which the caller reserves
static int mvs_view_runs(srh_context *c, const int32_t *slots, int nviews, DevBuf<double> ViewHost::*scratch, std::vector<MvsRun> &runs)
{
	int rc;
	for (int i = 0; i < nviews; ++i) {
		if ((rc = check_slot(c, slots[i], true))) return rc;
		if (c->views[slots[i]].peaks_k < 1) return fail(SRH_E_INVALID, "view slot %d has no peaks (srh_mvs_initial_estimate_peaks first)", slots[i]);
		for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return fail(SRH_E_INVALID, "view slot %d listed twice", slots[i]);
	}
	HIP_TRY(hipSetDevice(c->device));
	if (!c->views_go) HIP_TRY(hipEventCreateWithFlags(&c->views_go, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(c->views_go, c->stream));
	for (int i = 0; i < nviews; ++i) {
		ViewHost &v = c->views[slots[i]];
		if (!c->mrf_stream[i]) HIP_TRY(hipStreamCreateWithFlags(&c->mrf_stream[i], hipStreamNonBlocking));
		HIP_TRY(hipStreamWaitEvent(c->mrf_stream[i], c->views_go, 0));
		runs.push_back(MvsRun{ slots[i], v.w, v.h, v.peaks_k, c->mrf_stream[i], &(v.*scratch), v.peaks });
	}
	return SRH_OK;
}

// TRW-S on every run (their scratch is reserved here, without a pre-check), each by the reference's stopping rule for itself (multiviewstereo.cpp:627-641): sweeps while the
// energy drops by more than min_energy_drop, max_iters + 1 at the most.  A round queues the next step of every run still
// sweeping -- the set-up in round 0, then a sweep; behind it the energy of the labelling it leaves and that number's way
// to the host -- before it waits for the first, so runs side by side overlap.  `prof`: profile entries (the one-view form's).
static int mvs_mrf_drive(srh_context *c, int n, const MvsRun *runs, const srh_mrf_params *m, srh_mrf_info *infos, bool prof)
{
	struct HostState { double energy, pad; unsigned status[4]; };
	for (int i = 0; i < n; ++i) if (const int rc = runs[i].scratch->ensure(mrf_scratch_doubles(runs[i].w, runs[i].h))) return rc;
	if (!c->mrf_host) HIP_TRY(hipHostMalloc(&c->mrf_host, sizeof(HostState)*SRH_MAX_VIEWS, hipHostMallocDefault));
	HostState *hs = static_cast<HostState *>(c->mrf_host);
	struct Live { MrfLayout lay; double e = 0, prev = 0, e0 = 0; int iters = 0, left = 0; bool active = true; };
	std::vector<Live> live(n);
	auto stop = [&](int code) { for (int i = 0; i < n; ++i) hipStreamSynchronize(runs[i].st); return code; };
	auto failed = [&](int i) { return stop(fail(SRH_E_DEVICE, "MRF of view slot %d failed after %d sweep(s): %s", runs[i].slot, live[i].iters,
	                                            hipGetErrorString(hipGetLastError()))); };
	for (int nactive = n, round = 0; nactive > 0; ++round) {
		if (round && cancelled(c)) return stop(fail(SRH_E_CANCELLED, "cancelled"));
		for (int i = 0; i < n; ++i) {
			const MvsRun &r = runs[i]; Live &l = live[i];
			if (!l.active) continue;
			hipError_t e;
			if (round == 0) { Scope s(c, c->stream, "mrf_data_kernel", prof); e = launch_mrf_setup(r.st, *r.scratch, r.w, r.h, r.K, m->beta, m->lambda, m->phi_u, r.peaks, l.lay); }
			else            { Scope s(c, c->stream, "mrf_pass_kernel", prof); e = launch_mrf_sweep(r.st, *r.scratch, r.w, r.h, r.K, m->psi_u, l.iters); }
			if (e == hipSuccess) { Scope s(c, c->stream, "mrf_energy_kernel", prof); e = launch_mrf_energy(r.st, *r.scratch, r.w, r.h, r.K, m->psi_u); }
			if (e == hipSuccess) e = hipMemcpyAsync(&hs[i], l.lay.energy, sizeof(HostState), hipMemcpyDeviceToHost, r.st);
			if (e != hipSuccess) return failed(i);
		}
		for (int i = 0; i < n; ++i) {
			const MvsRun &r = runs[i]; Live &l = live[i];
			if (!l.active) continue;
			if (hipStreamSynchronize(r.st) != hipSuccess) return failed(i);
			if (hs[i].status[0])
				return stop(fail(SRH_E_DEVICE, "MRF sweep %u of view slot %d: band %u waited too long for the band above (hand-off never arrived)",
				                 hs[i].status[2], r.slot, hs[i].status[1] - 1));
			l.prev = l.e; l.e = hs[i].energy;
			if (round == 0) { l.e0 = l.e; l.left = m->max_iters; continue; }
			++l.iters;
			if (l.prev - l.e > m->min_energy_drop && l.left-- > 0) continue;     // do { ... } while (prev - energy > 5 && numIters-- > 0)
			l.active = false; --nactive;
			Scope s(c, c->stream, "mrf_depth_kernel", prof);
			if (launch_mrf_depth(r.st, c->d_views, r.slot, *r.scratch, r.w, r.h, r.K) != hipSuccess) return failed(i);
		}
	}
	for (int i = 0; i < n; ++i) {
		if (hipStreamSynchronize(runs[i].st) != hipSuccess) return failed(i);
		if (infos) { infos[i].iterations = live[i].iters; infos[i].energy_initial = live[i].e0; infos[i].energy_final = live[i].e; }
	}
	return SRH_OK;
}

extern "C" int srh_mvs_mrf_estimate(srh_context *c, int slot, int K, const void *peaks_dev, const srh_mrf_params *m, srh_mrf_info *info)
{
	int rc;
	if ((rc = check_slot(c, slot, true))) return rc;
	if (!peaks_dev || !m) return fail(SRH_E_INVALID, "null peaks / params");
	if (K < 1 || K > 15) return fail(SRH_E_UNSUPPORTED, "top_k %d outside [1,15] (one lane per label, 16 lanes per pixel)", K);
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	c->mrf.forget();
	const MvsRun run = { slot, v.w, v.h, K, c->stream, &c->mrf.scratch, static_cast<const double *>(peaks_dev) };
	if ((rc = mvs_mrf_drive(c, 1, &run, m, info, true))) return rc;
	c->mrf.finished(v.w, v.h, K);
	return SRH_OK;
}

extern "C" int srh_mvs_initial_estimate_mrf(srh_context *c, int slot, const int32_t *neigh, int nneigh, const srh_params *p,
                                            const srh_mrf_params *m, srh_mrf_info *info)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	if (!m) return fail(SRH_E_INVALID, "null MRF params");
	if (p->top_k < 1 || p->top_k > 15) return fail(SRH_E_UNSUPPORTED, "top_k %d outside [1,15]", p->top_k);
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if ((rc = c->mrf_peaks.ensure((size_t)v.w*v.h*p->top_k*2))) return rc;
	if ((rc = srh_mvs_initial_estimate(c, slot, neigh, nneigh, p, 0, 0, c->mrf_peaks))) return rc;
	return srh_mvs_mrf_estimate(c, slot, p->top_k, c->mrf_peaks, m, info);
}

extern "C" int srh_mvs_initial_estimate_peaks(srh_context *c, int slot, const int32_t *neigh, int nneigh, const srh_params *p)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	if (p->top_k < 1 || p->top_k > 15) return fail(SRH_E_UNSUPPORTED, "top_k %d outside [1,15]", p->top_k);
	HIP_TRY(hipSetDevice(c->device));
	ViewHost &v = c->views[slot];
	v.peaks_k = 0;
	if ((rc = v.peaks.ensure((size_t)v.w*v.h*p->top_k*2))) return rc;
	if ((rc = srh_mvs_initial_estimate(c, slot, neigh, nneigh, p, 0, 0, v.peaks))) return rc;
	v.peaks_k = p->top_k;
	return SRH_OK;
}

// The MRF stage of several views at once.  A sweep occupies one workgroup per 16 image rows and is bound by its own
// dependency chain (60 of 256 CUs at 1280x960), so the views' sweeps run side by side, each on a stream of its own with
// its own scratch; every view keeps the reference's stopping rule for itself (multiviewstereo.cpp:627-641).
extern "C" int srh_mvs_mrf_estimate_views(srh_context *c, const int32_t *slots, int nviews, const srh_mrf_params *m, srh_mrf_info *infos)
{
	int rc;
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (!slots || nviews < 1 || nviews > SRH_MAX_VIEWS || !m) return fail(SRH_E_INVALID, "bad view list / params");
	std::vector<MvsRun> runs;
	if ((rc = mvs_view_runs(c, slots, nviews, &ViewHost::mrf, runs))) return rc;
	c->mrf.forget();                                          // the per-view runs leave no state srh_mvs_mrf_state could report
	return mvs_mrf_drive(c, nviews, runs.data(), m, infos, false);
}

extern "C" int srh_mvs_mrf_dims(srh_context *c, int *w, int *h, int *top_k)
{
	return !c ? fail(SRH_E_INVALID, "null context") : c->mrf.dims(w, h, top_k);
}

extern "C" int srh_mvs_mrf_state(srh_context *c, int bw, int bh, int bk, int32_t *labels, double *data_costs, double *messages)
{
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (const int rc = c->mrf.check_dims(bw, bh, bk)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const int w = c->mrf.w, h = c->mrf.h, K = c->mrf.l, L = K + 1;
	const size_t n = (size_t)w*h;
	MrfLayout lay;
	launch_mrf_layout(c->mrf.scratch, w, h, lay);
	if (labels) HIP_TRY(hipMemcpyAsync(labels, lay.ans, n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	// device rows are 16 labels wide: copy the first L of each
	if (data_costs) HIP_TRY(hipMemcpy2DAsync(data_costs, L*sizeof(double), lay.D, 16*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
	if (messages) {
		HIP_TRY(hipMemcpy2DAsync(messages, 2*L*sizeof(double), lay.Mh, 16*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipMemcpy2DAsync(messages + L, 2*L*sizeof(double), lay.Mv, 16*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
	}
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// ------------------------------------------------------------------ MultiViewStereo, semi-global aggregation (srh_mvs_sgm.hip)
extern "C" void srh_mvs_sgm_params_defaults(srh_mvs_sgm_params *m)
{
	if (!m) return;
	m->beta = 1; m->lambda = 1; m->phi_u = 0.5; m->psi_u = 0.002;     // the MRF branch's
	m->path_mask = 0xFF;
}

static int check_mvsgm_params(const srh_mvs_sgm_params *m)
{
	if (!m) return fail(SRH_E_INVALID, "null SGM params");
	if (!(m->lambda >= 0 && m->phi_u >= 0 && m->psi_u >= 0)) return fail(SRH_E_INVALID, "lambda %g, phi_u %g, psi_u %g must be >= 0", m->lambda, m->phi_u, m->psi_u);
	if (!(m->beta > -__builtin_inf() && m->beta < __builtin_inf())) return fail(SRH_E_INVALID, "beta %g must be finite", m->beta);
	if (m->path_mask <= 0 || m->path_mask > 0xFF) return fail(SRH_E_INVALID, "path_mask 0x%x: bits 0..7 enable the 8 directions, at least one", (unsigned)m->path_mask);
	return SRH_OK;
}

// The aggregation on every run, after the pre-check of all their scratch: everything is queued direction by direction for
// all of them, and the host waits once, at the end.  `prof`: profile entries (the one-view form's).
static int mvs_sgm_drive(srh_context *c, int n, const MvsRun *runs, const srh_mvs_sgm_params *m, srh_sgm_info *infos, bool prof)
{
	// (a profile entry per direction: rows, columns and diagonals stream differently)
	static const char *const names[8] = { "mvs_sgm_path_kernel[+1,0]", "mvs_sgm_path_kernel[-1,0]", "mvs_sgm_path_kernel[0,+1]",
	                                      "mvs_sgm_path_kernel[0,-1]", "mvs_sgm_path_kernel[+1,+1]", "mvs_sgm_path_kernel[-1,-1]",
	                                      "mvs_sgm_path_kernel[+1,-1]", "mvs_sgm_path_kernel[-1,+1]" };
	int rc;
	std::vector<StageWant> wants;
	for (int i = 0; i < n; ++i) wants.push_back({ runs[i].scratch, mvs_sgm_scratch_doubles(runs[i].w, runs[i].h) });
	if ((rc = stage_reserve(c, wants.data(), n, [&](size_t need, size_t avail) {
		return fail(SRH_E_DEVICE, "the semi-global aggregation of %d view(s) (the first %dx%d) needs %zu bytes of device memory (per view peak depths, data costs and sums, %zu each at 16 doubles per pixel, + the labels; no bands: a path crosses the whole grid), %zu are available",
		            n, runs[0].w, runs[0].h, need, (size_t)runs[0].w*runs[0].h*16*sizeof(double), avail); }))) return rc;
	if (!c->mvsgm_host) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c->mvsgm_host), sizeof(double)*SRH_MAX_VIEWS, hipHostMallocDefault));
	auto stop = [&](int code) { for (int i = 0; i < n; ++i) hipStreamSynchronize(runs[i].st); return code; };
	auto failed = [&](const char *what, int i) { return stop(fail(SRH_E_DEVICE, "SGM %s of view slot %d failed: %s", what, runs[i].slot,
	                                                              hipGetErrorString(hipGetLastError()))); };
	for (int i = 0; i < n; ++i) {
		const MvsRun &r = runs[i];
		Scope s(c, c->stream, "mrf_data_kernel", prof);
		if (launch_mvs_sgm_setup(r.st, *r.scratch, r.w, r.h, r.K, m->beta, m->lambda, m->phi_u, r.peaks) != hipSuccess) return failed("setup", i);
	}
	int paths = 0;
	for (int k = 0; k < 8; ++k) {
		if (!(m->path_mask >> k & 1)) continue;
		// (nothing of a slot has been written yet: the depth map is the read-off's, after the last direction)
		if (cancelled(c)) return stop(fail(SRH_E_CANCELLED, "cancelled"));
		for (int i = 0; i < n; ++i) {
			const MvsRun &r = runs[i];
			Scope s(c, c->stream, names[k], prof);
			if (launch_mvs_sgm_path(r.st, *r.scratch, r.w, r.h, r.K, m->psi_u, k, paths == 0) != hipSuccess) return failed("path", i);
		}
		++paths;
	}
	for (int i = 0; i < n; ++i) {
		const MvsRun &r = runs[i];
		MvsSgmLayout lay;
		mvs_sgm_layout(*r.scratch, r.w, r.h, lay);
		hipError_t e;
		{ Scope s(c, c->stream, "mvs_sgm_readoff_kernel", prof); e = launch_mvs_sgm_readoff(r.st, c->d_views, r.slot, *r.scratch, r.w, r.h, r.K); }
		if (e == hipSuccess) { Scope s(c, c->stream, "mrf_energy_kernel", prof); e = launch_mvs_sgm_energy(r.st, *r.scratch, r.w, r.h, r.K, m->psi_u); }
		if (e == hipSuccess) e = hipMemcpyAsync(&c->mvsgm_host[i], lay.energy, sizeof(double), hipMemcpyDeviceToHost, r.st);
		if (e != hipSuccess) return failed("read-off", i);
	}
	for (int i = 0; i < n; ++i) {
		if (hipStreamSynchronize(runs[i].st) != hipSuccess) return failed("read-off", i);
		if (infos) { infos[i].paths = paths; infos[i].energy = c->mvsgm_host[i]; }
	}
	return SRH_OK;
}

extern "C" int srh_mvs_sgm_estimate(srh_context *c, int slot, int K, const void *peaks_dev, const srh_mvs_sgm_params *m, srh_sgm_info *info)
{
	int rc;
	if ((rc = check_slot(c, slot, true))) return rc;
	if (!peaks_dev || !m) return fail(SRH_E_INVALID, "null peaks / params");
	if (K < 1 || K > 15) return fail(SRH_E_UNSUPPORTED, "top_k %d outside [1,15] (one lane per label, 16 lanes per pixel)", K);
	if ((rc = check_mvsgm_params(m))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	c->mvsgm.forget();
	const MvsRun run = { slot, v.w, v.h, K, c->stream, &c->mvsgm.scratch, static_cast<const double *>(peaks_dev) };
	if ((rc = mvs_sgm_drive(c, 1, &run, m, info, true))) return rc;
	c->mvsgm.finished(v.w, v.h, K);
	return SRH_OK;
}

extern "C" int srh_mvs_initial_estimate_sgm(srh_context *c, int slot, const int32_t *neigh, int nneigh, const srh_params *p,
                                            const srh_mvs_sgm_params *m, srh_sgm_info *info)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	if (!m) return fail(SRH_E_INVALID, "null SGM params");
	if (p->top_k < 1 || p->top_k > 15) return fail(SRH_E_UNSUPPORTED, "top_k %d outside [1,15]", p->top_k);
	if ((rc = check_mvsgm_params(m))) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if ((rc = c->mrf_peaks.ensure((size_t)v.w*v.h*p->top_k*2))) return rc;
	if ((rc = srh_mvs_initial_estimate(c, slot, neigh, nneigh, p, 0, 0, c->mrf_peaks))) return rc;
	return srh_mvs_sgm_estimate(c, slot, p->top_k, c->mrf_peaks, m, info);
}

// The aggregation of several views at once.  One direction of one 1280x960 view is a few hundred waves' worth of lines on a
// chip of 1024 SIMDs, so the views run side by side, each on a stream of its own (the MRF branch's) with its own scratch:
// everything is queued direction by direction, and the host waits once, at the end.
extern "C" int srh_mvs_sgm_estimate_views(srh_context *c, const int32_t *slots, int nviews, const srh_mvs_sgm_params *m, srh_sgm_info *infos)
{
	int rc;
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (!slots || nviews < 1 || nviews > SRH_MAX_VIEWS || !m) return fail(SRH_E_INVALID, "bad view list / params");
	if ((rc = check_mvsgm_params(m))) return rc;
	std::vector<MvsRun> runs;
	if ((rc = mvs_view_runs(c, slots, nviews, &ViewHost::sgm, runs))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	c->mvsgm.forget();                                        // the per-view runs leave no state srh_mvs_sgm_state could report
	return mvs_sgm_drive(c, nviews, runs.data(), m, infos, false);
}

extern "C" int srh_mvs_sgm_dims(srh_context *c, int *w, int *h, int *top_k)
{
	return !c ? fail(SRH_E_INVALID, "null context") : c->mvsgm.dims(w, h, top_k);
}

extern "C" int srh_mvs_sgm_state(srh_context *c, int bw, int bh, int bk, int32_t *labels, double *data_costs, double *sums)
{
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (const int rc = c->mvsgm.check_dims(bw, bh, bk)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	const int w = c->mvsgm.w, h = c->mvsgm.h, K = c->mvsgm.l, L = K + 1;
	const size_t n = (size_t)w*h;
	MvsSgmLayout lay;
	mvs_sgm_layout(c->mvsgm.scratch, w, h, lay);
	if (labels) HIP_TRY(hipMemcpyAsync(labels, lay.ans, n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	// device rows are 16 labels wide: copy the first L of each
	if (data_costs) HIP_TRY(hipMemcpy2DAsync(data_costs, L*sizeof(double), lay.D, 16*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
	if (sums) HIP_TRY(hipMemcpy2DAsync(sums, L*sizeof(double), lay.S, 16*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// ------------------------------------------------------------------ TwoViewStereo, MRF stage (srh_twoview_mrf.hip)
extern "C" void srh_twoview_mrf_params_defaults(srh_twoview_mrf_params *m)
{
	if (!m) return;
	m->smooth_exp = 1; m->smooth_max = 2; m->lambda = 0.25;          // twoviewstereo.cpp:69-71
	m->max_iters = 50; m->min_energy_drop = 5;                       // :378, :390
}

// the label count and the smoothness term of a TwoView label stage: the optimiser and the aggregation take the same
template <class Params>
static int check_tv_smoothness(const Params *m, int L, const char *stage)
{
	if (!m) return fail(SRH_E_INVALID, "null %s params", stage);
	if (L < 2 || L > 256) return fail(SRH_E_UNSUPPORTED, "%d labels outside [2,256] (64 lanes per pixel, up to 4 labels per lane)", L);
	if (m->smooth_exp != 1) return fail(SRH_E_UNSUPPORTED, "smooth_exp %d: only the truncated-linear term (1) is built", m->smooth_exp);
	if (!(m->smooth_max > 0 && m->smooth_max <= 4)) return fail(SRH_E_UNSUPPORTED, "smooth_max %g outside (0,4] (the message window reaches 3 labels)", m->smooth_max);
	if (!(m->lambda >= 0 && m->lambda < __builtin_inf())) return fail(SRH_E_INVALID, "lambda %g must be finite and >= 0", m->lambda);
	return SRH_OK;
}

static int check_tvmrf_params(const srh_twoview_mrf_params *m, int L)
{
	if (const int rc = check_tv_smoothness(m, L, "MRF")) return rc;
	if (m->max_iters < 0 || m->max_iters > (1 << 24)) return fail(SRH_E_INVALID, "max_iters %d outside [0,2^24]", m->max_iters);
	return SRH_OK;
}

// What tells the two TwoView label stages apart outside their runs: the state, the scratch's size, the words of the
// pre-check's refusal (tv_stage_reserve) and the name of the stage's step in srh_twoview_compute_*'s progress
struct TvStage { LabelStage srh_context::*state; size_t (*scratch_doubles)(int w, int h, int L); const char *what, *planes, *why, *progress; };
static const TvStage TV_MRF = { &srh_context::tvmrf, twoview_mrf_scratch_doubles, "MRF stage", "two message planes", "sweep needs", "Optimizing..." };
static const TvStage TV_SGM = { &srh_context::tvsgm, twoview_sgm_scratch_doubles, "semi-global aggregation", "sums", "path crosses", "Aggregating..." };

// a new run of the stage on a w x h x L volume: its scratch, and its own cost volume when the costs are not the caller's
static int tv_stage_reserve(srh_context *c, const TvStage &T, int w, int h, int L, bool own_costs)
{
	LabelStage &S = c->*T.state;
	S.forget();
	const size_t vol = (size_t)w*h*L;
	const StageWant wants[2] = { { &S.scratch, T.scratch_doubles(w, h, L) }, { &S.costs, own_costs ? vol : 0 } };
	S.own_costs = own_costs;
	return stage_reserve(c, wants, 2, [&](size_t need, size_t avail) {
		return fail(SRH_E_DEVICE, "the %s of a %dx%dx%d volume needs %zu bytes of device memory (%s%s: %zu per volume, no bands: a %s the whole grid), %zu are available",
		            T.what, w, h, L, need, own_costs ? "costs and " : "", T.planes, vol*sizeof(double), T.why, avail);
	});
}

// the label cost volume of ref against oth into the stage's own buffer
static int tv_stage_costs(srh_context *c, const TvStage &T, int ref, int oth, const srh_params *p)
{
	int rc;
	const ViewHost &v = c->views[ref];
	if ((rc = tv_stage_reserve(c, T, v.w, v.h, p->num_depth_levels, true))) return rc;
	if (c->cost_kind == SRH_COST_CENSUS && ((rc = ensure_census(c, c->stream, ref)) || (rc = ensure_census(c, c->stream, oth)))) return rc;
	Scope s(c, c->stream, "twoview_label_costs_kernel");
	HIP_TRY(launch_twoview_label_costs(c->stream, c->d_views, ref, oth, v.w, *p, c->cost_kind, 0, v.h,
	                                   (2*p->window_radius + 1)*p->bad_ret, (c->*T.state).costs, nullptr));
	return SRH_OK;
}

// srh_twoview_compute_mrf / _sgm: both directions through the stage, run(ref, k) on its own cost volume, then the end of
// srh_twoview_compute.  Progress steps as a USE_MRF build of TwoViewStereo emits them (twoviewstereo.cpp:234, 337, 405, 506, 597, 225).
template <class Run>
static int tv_stage_compute(srh_context *c, const TvStage &T, int left, int right, const srh_params *p, double *left_out, double *right_out, Run run)
{
	int rc;
	const ViewHost &L = c->views[left], &Rv = c->views[right];
	if (L.w != Rv.w || L.h != Rv.h) return fail(SRH_E_INVALID, "TwoViewStereo needs equal-sized views");
	if (c->filter_invalid && ((rc = check_filter(c, left, p, c->filter_invalid)) || (rc = check_filter(c, right, p, c->filter_invalid)))) return rc;
	if (c->speckle_min_size && (rc = check_twoview_speckles(c, left, right, p))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	for (int k = 0; k < 2; ++k) {
		const int ref = k == 0 ? left : right, oth = k == 0 ? right : left;
		progress(c, 1 + 2*k, k == 0 ? "Computing cost volume for left image..." : "Computing cost volume for right image...");
		HIP_TRY(hipSetDevice(c->device));
		if ((rc = tv_stage_costs(c, T, ref, oth, p))) return rc;
		// (the cost kernel is queued: a cancelled call returns with the stream idle, as everywhere else)
		if (cancelled(c)) { HIP_TRY(hipStreamSynchronize(c->stream)); return fail(SRH_E_CANCELLED, "cancelled"); }
		progress(c, 2 + 2*k, T.progress);
		if ((rc = run(ref, k))) return rc;
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	}
	progress(c, 5, "Detecting inconsistencies...");
	if ((rc = srh_twoview_cross_check(c, left, right, p))) return rc;
	if (c->speckle_min_size && (rc = twoview_speckles(c, left, right, p))) return rc;
	if (c->filter_invalid && (rc = twoview_filter(c, left, right, p))) return rc;
	if (left_out && (rc = srh_view_depth_download(c, left, left_out))) return rc;
	if (right_out && (rc = srh_view_depth_download(c, right, right_out))) return rc;
	if ((rc = srh_synchronize(c))) return rc;
	progress(c, 8, "Finished!");
	return SRH_OK;
}

// the optimiser on `costs` (device, [pixel][L]); the scratch is reserved
static int tvmrf_run(srh_context *c, int slot, const srh_params *p, int L, const double *costs, const srh_twoview_mrf_params *m, srh_mrf_info *info)
{
	int rc;
	ViewHost &v = c->views[slot];
	const int w = v.w, h = v.h;
	c->tvmrf.forget();
	v.wta_flags = 0;                                            // no scan made this depth map: the WTA by-products are stale
	TvMrfLayout lay;
	HIP_TRY(launch_twoview_mrf_setup(c->stream, c->tvmrf.scratch, w, h, L, lay));
	struct { double energy, pad; unsigned status[4]; } hs;
	auto energy = [&](double &e) -> int {
		{ Scope s(c, c->stream, "twoview_mrf_energy_kernel");
		  HIP_TRY(launch_twoview_mrf_energy(c->stream, c->tvmrf.scratch, costs, w, h, L, m->lambda, m->smooth_max)); }
		HIP_TRY(hipMemcpyAsync(&hs, lay.energy, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if (hs.status[0])
			return fail(SRH_E_DEVICE, "TwoView MRF pass %u: band %u waited too long for the band above (hand-off never arrived)", hs.status[2], hs.status[1] - 1);
		e = hs.energy;
		return SRH_OK;
	};
	// twoviewstereo.cpp:378-390
	double e = 0.0, prev = 0.0;
	if ((rc = energy(e))) return rc;
	const double e0 = e;
	int num_iters = m->max_iters, iters = 0;
	do {
		if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
		prev = e;
		{ Scope s(c, c->stream, "twoview_mrf_pass_kernel");
		  HIP_TRY(launch_twoview_mrf_sweep(c->stream, c->tvmrf.scratch, costs, w, h, L, m->lambda, m->smooth_max, iters)); }
		if ((rc = energy(e))) return rc;
		++iters;
	} while (prev - e > m->min_energy_drop && num_iters-- > 0);
	{ Scope s(c, c->stream, "twoview_mrf_depth_kernel");
	  HIP_TRY(launch_twoview_mrf_depth(c->stream, c->d_views, slot, *p, c->tvmrf.scratch, w, h, L)); }
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->tvmrf.finished(w, h, L);
	if (info) { info->iterations = iters; info->energy_initial = e0; info->energy_final = e; }
	return SRH_OK;
}

extern "C" int srh_twoview_mrf_optimize(srh_context *c, int slot, const srh_params *p, int L, const void *costs_dev,
                                        const srh_twoview_mrf_params *m, srh_mrf_info *info)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	if (!costs_dev) return fail(SRH_E_INVALID, "null cost volume");
	if ((rc = check_tvmrf_params(m, L))) return rc;
	if (L != p->num_depth_levels) return fail(SRH_E_INVALID, "%d labels, but num_depth_levels is %d (depthFromLabel needs the label count)", L, p->num_depth_levels);
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if ((rc = tv_stage_reserve(c, TV_MRF, v.w, v.h, L, false))) return rc;
	return tvmrf_run(c, slot, p, L, static_cast<const double *>(costs_dev), m, info);
}

static int check_label_costs(srh_context *c, int ref, int oth, const srh_params *p)
{
	int rc;
	if ((rc = check_slot(c, ref, true)) || (rc = check_slot(c, oth, true)) || (rc = check_params(p))) return rc;
	if (ref == oth) return fail(SRH_E_INVALID, "ref and other view are the same slot");
	if (p->window_radius > 5) return fail(SRH_E_UNSUPPORTED, "label costs take window radii up to 5");
	return SRH_OK;
}

extern "C" int srh_twoview_label_costs(srh_context *c, int ref, int oth, const srh_params *p, int y0, int y1,
                                       double *cost_out, int32_t *pixel_out)
{
	int rc;
	if ((rc = check_label_costs(c, ref, oth, p))) return rc;
	if (!cost_out) return fail(SRH_E_INVALID, "null cost output");
	const ViewHost &v = c->views[ref];
	if (y1 <= 0) y1 = v.h;
	if (y0 < 0 || y0 >= y1 || y1 > v.h) return fail(SRH_E_INVALID, "rows [%d,%d) outside the view's %d rows", y0, y1, v.h);
	HIP_TRY(hipSetDevice(c->device));
	if (c->cost_kind == SRH_COST_CENSUS) {
		int rc;
		if ((rc = ensure_census(c, c->stream, ref)) || (rc = ensure_census(c, c->stream, oth))) return rc;
	}
	const int D = p->num_depth_levels;
	const size_t n = (size_t)(y1 - y0)*v.w*D;
	DevBuf<double> dcost; DevBuf<int32_t> dpix;
	auto done = [&](int r) { dcost.free(); dpix.free(); return r; };
	if (dcost.alloc(n) != hipSuccess || (pixel_out && dpix.alloc(2*n) != hipSuccess))
		return done(fail(SRH_E_DEVICE, "label costs: no device memory for %zu bytes", n*(sizeof(double) + (pixel_out ? 2*sizeof(int32_t) : 0))));
	hipError_t e;
	{ Scope s(c, c->stream, "twoview_label_costs_kernel");
	  e = launch_twoview_label_costs(c->stream, c->d_views, ref, oth, v.w, *p, c->cost_kind, y0, y1 - y0,
	                                 (2*p->window_radius + 1)*p->bad_ret, dcost, pixel_out ? (int32_t *)dpix : nullptr); }
	if (e == hipSuccess) e = hipMemcpyAsync(cost_out, dcost, n*sizeof(double), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess && pixel_out) e = hipMemcpyAsync(pixel_out, dpix, 2*n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) return done(fail(SRH_E_DEVICE, "label costs: %s", hipGetErrorString(e)));
	return done(SRH_OK);
}

extern "C" int srh_twoview_mrf(srh_context *c, int ref, int oth, const srh_params *p, const srh_twoview_mrf_params *m, srh_mrf_info *info)
{
	int rc;
	if ((rc = check_label_costs(c, ref, oth, p))) return rc;
	const int L = p->num_depth_levels;
	if ((rc = check_tvmrf_params(m, L))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	HIP_TRY(hipSetDevice(c->device));
	if ((rc = tv_stage_costs(c, TV_MRF, ref, oth, p))) return rc;
	return tvmrf_run(c, ref, p, L, c->tvmrf.costs, m, info);
}

extern "C" int srh_twoview_compute_mrf(srh_context *c, int left, int right, const srh_params *p, const srh_twoview_mrf_params *m,
                                       double *left_out, double *right_out, srh_mrf_info *infos)
{
	int rc;
	if ((rc = check_label_costs(c, left, right, p))) return rc;
	if ((rc = check_tvmrf_params(m, p->num_depth_levels))) return rc;
	return tv_stage_compute(c, TV_MRF, left, right, p, left_out, right_out, [&](int ref, int k) {
		return tvmrf_run(c, ref, p, p->num_depth_levels, c->tvmrf.costs, m, infos ? infos + k : nullptr);
	});
}

extern "C" int srh_twoview_mrf_dims(srh_context *c, int *w, int *h, int *L)
{
	return !c ? fail(SRH_E_INVALID, "null context") : c->tvmrf.dims(w, h, L);
}

extern "C" int srh_twoview_mrf_state(srh_context *c, int bw, int bh, int bl, int32_t *labels, double *data_costs, double *messages)
{
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (const int rc = c->tvmrf.check_dims(bw, bh, bl)) return rc;
	if (data_costs && !c->tvmrf.own_costs)
		return fail(SRH_E_INVALID, "the data costs of srh_twoview_mrf_optimize are the caller's volume: the context keeps none");
	HIP_TRY(hipSetDevice(c->device));
	const int w = c->tvmrf.w, h = c->tvmrf.h, L = c->tvmrf.l;
	const size_t n = (size_t)w*h;
	TvMrfLayout lay;
	launch_twoview_mrf_layout(c->tvmrf.scratch, w, h, L, lay);
	if (labels) HIP_TRY(hipMemcpyAsync(labels, lay.ans, n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	if (data_costs) HIP_TRY(hipMemcpyAsync(data_costs, c->tvmrf.costs, n*L*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (messages) {
		HIP_TRY(hipMemcpy2DAsync(messages, 2*L*sizeof(double), lay.Mh, L*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipMemcpy2DAsync(messages + L, 2*L*sizeof(double), lay.Mv, L*sizeof(double), L*sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
	}
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// ------------------------------------------------------------------ TwoViewStereo, semi-global aggregation (srh_twoview_sgm.hip)
extern "C" void srh_twoview_sgm_params_defaults(srh_twoview_sgm_params *m)
{
	if (!m) return;
	m->smooth_exp = 1; m->smooth_max = 2; m->lambda = 0.25;          // the MRF stage's smoothness term
	m->path_mask = 0xFF;
}

static int check_tvsgm_params(const srh_twoview_sgm_params *m, int L)
{
	if (const int rc = check_tv_smoothness(m, L, "SGM")) return rc;
	if (m->path_mask <= 0 || m->path_mask > 0xFF) return fail(SRH_E_INVALID, "path_mask 0x%x: bits 0..7 enable the 8 directions, at least one", (unsigned)m->path_mask);
	return SRH_OK;
}

// the aggregation on `costs` (device, [pixel][L]); the scratch is reserved
static int tvsgm_run(srh_context *c, int slot, const srh_params *p, int L, const double *costs, const srh_twoview_sgm_params *m, srh_sgm_info *info)
{
	ViewHost &v = c->views[slot];
	const int w = v.w, h = v.h;
	c->tvsgm.forget();
	TvSgmLayout lay;
	twoview_sgm_layout(c->tvsgm.scratch, w, h, L, lay);
	// (a profile entry per direction: rows, columns and diagonals stream differently)
	static const char *const names[8] = { "twoview_sgm_path_kernel[+1,0]", "twoview_sgm_path_kernel[-1,0]", "twoview_sgm_path_kernel[0,+1]",
	                                      "twoview_sgm_path_kernel[0,-1]", "twoview_sgm_path_kernel[+1,+1]", "twoview_sgm_path_kernel[-1,-1]",
	                                      "twoview_sgm_path_kernel[+1,-1]", "twoview_sgm_path_kernel[-1,+1]" };
	int paths = 0;
	for (int k = 0; k < 8; ++k) {
		if (!(m->path_mask >> k & 1)) continue;
		// (nothing of the slot has been written yet: the depth map is the read-off's, after the last direction)
		if (cancelled(c)) { HIP_TRY(hipStreamSynchronize(c->stream)); return fail(SRH_E_CANCELLED, "cancelled"); }
		{ Scope s(c, c->stream, names[k]);
		  HIP_TRY(launch_twoview_sgm_path(c->stream, c->tvsgm.scratch, costs, w, h, L, m->lambda, m->smooth_max, k, paths == 0)); }
		++paths;
	}
	v.wta_flags = 0;                                            // no scan made this depth map: the WTA by-products are stale
	{ Scope s(c, c->stream, "twoview_sgm_readoff_kernel");
	  HIP_TRY(launch_twoview_sgm_readoff(c->stream, c->d_views, slot, *p, c->tvsgm.scratch, w, h, L)); }
	{ Scope s(c, c->stream, "twoview_mrf_energy_kernel");
	  HIP_TRY(launch_twoview_sgm_energy(c->stream, c->tvsgm.scratch, costs, w, h, L, m->lambda, m->smooth_max)); }
	double e = 0.0;
	HIP_TRY(hipMemcpyAsync(&e, lay.energy, sizeof(e), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->tvsgm.finished(w, h, L);
	if (info) { info->paths = paths; info->energy = e; }
	return SRH_OK;
}

extern "C" int srh_twoview_sgm_aggregate(srh_context *c, int slot, const srh_params *p, int L, const void *costs_dev,
                                         const srh_twoview_sgm_params *m, srh_sgm_info *info)
{
	int rc;
	if ((rc = check_slot(c, slot, true)) || (rc = check_params(p))) return rc;
	if (!costs_dev) return fail(SRH_E_INVALID, "null cost volume");
	if ((rc = check_tvsgm_params(m, L))) return rc;
	if (L != p->num_depth_levels) return fail(SRH_E_INVALID, "%d labels, but num_depth_levels is %d (depthFromLabel needs the label count)", L, p->num_depth_levels);
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if ((rc = tv_stage_reserve(c, TV_SGM, v.w, v.h, L, false))) return rc;
	return tvsgm_run(c, slot, p, L, static_cast<const double *>(costs_dev), m, info);
}

extern "C" int srh_twoview_sgm(srh_context *c, int ref, int oth, const srh_params *p, const srh_twoview_sgm_params *m, srh_sgm_info *info)
{
	int rc;
	if ((rc = check_label_costs(c, ref, oth, p))) return rc;
	const int L = p->num_depth_levels;
	if ((rc = check_tvsgm_params(m, L))) return rc;
	if (cancelled(c)) return fail(SRH_E_CANCELLED, "cancelled");
	HIP_TRY(hipSetDevice(c->device));
	if ((rc = tv_stage_costs(c, TV_SGM, ref, oth, p))) return rc;
	return tvsgm_run(c, ref, p, L, c->tvsgm.costs, m, info);
}

extern "C" int srh_twoview_compute_sgm(srh_context *c, int left, int right, const srh_params *p, const srh_twoview_sgm_params *m,
                                       double *left_out, double *right_out, srh_sgm_info *infos)
{
	int rc;
	if ((rc = check_label_costs(c, left, right, p))) return rc;
	if ((rc = check_tvsgm_params(m, p->num_depth_levels))) return rc;
	return tv_stage_compute(c, TV_SGM, left, right, p, left_out, right_out, [&](int ref, int k) {
		return tvsgm_run(c, ref, p, p->num_depth_levels, c->tvsgm.costs, m, infos ? infos + k : nullptr);
	});
}

extern "C" int srh_twoview_sgm_dims(srh_context *c, int *w, int *h, int *L)
{
	return !c ? fail(SRH_E_INVALID, "null context") : c->tvsgm.dims(w, h, L);
}

extern "C" int srh_twoview_sgm_state(srh_context *c, int bw, int bh, int bl, int32_t *labels, double *data_costs, double *sums)
{
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (const int rc = c->tvsgm.check_dims(bw, bh, bl)) return rc;
	if (data_costs && !c->tvsgm.own_costs)
		return fail(SRH_E_INVALID, "the data costs of srh_twoview_sgm_aggregate are the caller's volume: the context keeps none");
	HIP_TRY(hipSetDevice(c->device));
	const int w = c->tvsgm.w, h = c->tvsgm.h, L = c->tvsgm.l;
	const size_t n = (size_t)w*h;
	TvSgmLayout lay;
	twoview_sgm_layout(c->tvsgm.scratch, w, h, L, lay);
	if (labels) HIP_TRY(hipMemcpyAsync(labels, lay.ans, n*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	if (data_costs) HIP_TRY(hipMemcpyAsync(data_costs, c->tvsgm.costs, n*L*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (sums) HIP_TRY(hipMemcpyAsync(sums, lay.S, n*L*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

// ------------------------------------------------------------------ GUI-side users of the camera model
extern "C" int srh_epipolar_preview(srh_context *c, int ref, int oth, double zmin, double zmax, int nd,
                                    int nq, const double *xy, double *out_xy, int32_t *counts)
{
	int rc;
	if ((rc = check_slot(c, ref, true)) || (rc = check_slot(c, oth, true))) return rc;
	if (nd < 2 || nq < 0 || (nq > 0 && (!xy || !out_xy || !counts))) return fail(SRH_E_INVALID, "bad preview arguments");
	if (nq == 0) return SRH_OK;
	HIP_TRY(hipSetDevice(c->device));
	const size_t nout = (size_t)nq*nd*2;
	// scratch in the band buffer: [xy | out | counts]
	if ((rc = c->mem.band.wbuf.ensure((size_t)2*nq + nout + (size_t)(nq + 1)/2 + 2))) return rc;
	double *d_xy = c->mem.band.wbuf, *d_out = c->mem.band.wbuf + 2*(size_t)nq;
	int32_t *d_cnt = reinterpret_cast<int32_t *>(d_out + nout);
	HIP_TRY(hipMemcpyAsync(d_xy, xy, (size_t)2*nq*sizeof(double), hipMemcpyHostToDevice, c->stream));
	{ Scope s(c, c->stream, "epipolar_preview_kernel");
	  launch_epipolar_preview(c->stream, c->d_views, ref, oth, zmin, zmax, nd, nq, d_xy, d_out, d_cnt); }
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out_xy, d_out, nout*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(counts, d_cnt, (size_t)nq*sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return SRH_OK;
}

extern "C" int srh_refraction_error(srh_context *c, int v1, int v2, int n, const double *p1, const double *p2,
                                    double *err_out, double *total, double *average)
{
	int rc;
	if ((rc = check_slot(c, v1, true)) || (rc = check_slot(c, v2, true))) return rc;
	if (n < 0 || (n > 0 && (!p1 || !p2))) return fail(SRH_E_INVALID, "bad correspondence arguments");
	HIP_TRY(hipSetDevice(c->device));
	std::vector<double> err((size_t)n);
	if (n > 0) {
		if ((rc = c->mem.band.wbuf.ensure((size_t)5*n))) return rc;
		double *d1 = c->mem.band.wbuf, *d2 = c->mem.band.wbuf + 2*(size_t)n, *de = c->mem.band.wbuf + 4*(size_t)n;
		HIP_TRY(hipMemcpyAsync(d1, p1, (size_t)2*n*sizeof(double), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d2, p2, (size_t)2*n*sizeof(double), hipMemcpyHostToDevice, c->stream));
		{ Scope s(c, c->stream, "refraction_error_kernel");
		  launch_refraction_error(c->stream, c->d_views, v1, v2, n, d1, d2, de); }
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(err.data(), de, (size_t)n*sizeof(double), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	double tot = 0.0;                                             // totalError: summed in correspondence order (:440)
	for (int i = 0; i < n; ++i) tot += err[i]*err[i];
	if (err_out) for (int i = 0; i < n; ++i) err_out[i] = err[i];
	if (total) *total = tot;
	if (average) *average = tot / n;
	return SRH_OK;
}

// ------------------------------------------------------------------ multi-GPU exchange
extern "C" int srh_comm_unique_id(void *id_out) {
	if (!id_out) return fail(SRH_E_INVALID, "null id buffer");
	if (const char *e = rccl_unique_id_get(id_out)) return fail(SRH_E_UNSUPPORTED, "RCCL: %s", e);
	return SRH_OK;
}

extern "C" int srh_comm_init(srh_context *c, int nranks, int rank, const void *id) {
	if (!c || !id) return fail(SRH_E_INVALID, "null argument");
	if (nranks < 1 || rank < 0 || rank >= nranks) return fail(SRH_E_INVALID, "rank %d of %d", rank, nranks);
	HIP_TRY(hipSetDevice(c->device));
	if (c->comm) { (void)rccl_comm_destroy(c->comm); c->comm = nullptr; }
	// librccl absent, or without the entry points this file needs: not a device failure (include/stereo_recon_hip.h)
	if (!rccl_available()) { c->comm_ranks = 0; return fail(SRH_E_UNSUPPORTED, "RCCL: librccl cannot be loaded"); }
	// (non-blocking communicator: a rank that never arrives is an error after the timeout, not a hang)
	if (const char *e = rccl_comm_init(&c->comm, nranks, rank, id)) { c->comm = nullptr; c->comm_ranks = 0; return fail(SRH_E_DEVICE, "RCCL: %s", e); }
	c->comm_ranks = nranks; c->comm_rank = rank;
	return SRH_OK;
}

// a collective that failed or timed out: the communicator is aborted (its peers' calls then fail too instead of
// waiting), the context has none until srh_comm_init is called again
static int comm_failed(srh_context *c, const char *what, const char *e) {
	const int rc = fail(SRH_E_DEVICE, "RCCL %s: %s", what, e);
	rccl_comm_abort(c->comm);
	c->comm = nullptr; c->comm_ranks = 0;
	return rc;
}

extern "C" int srh_comm_version(void) { return rccl_version(); }

extern "C" int srh_comm_set_timeout_ms(int ms) {
	if (ms <= 0) return fail(SRH_E_INVALID, "timeout must be > 0 ms");
	rccl_set_timeout_ms(ms);
	return SRH_OK;
}

extern "C" int srh_comm_info(srh_context *c, int *nranks, int *rank) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (nranks) *nranks = c->comm ? c->comm_ranks : 0;
	if (rank) *rank = c->comm ? c->comm_rank : -1;
	return SRH_OK;
}

extern "C" int srh_comm_gather_depth(srh_context *c, int slot, int root, void *recv_dev) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!c->comm) return fail(SRH_E_INVALID, "srh_comm_init has not been called");
	if (root < 0 || root >= c->comm_ranks) return fail(SRH_E_INVALID, "root %d of %d", root, c->comm_ranks);
	if (c->comm_rank == root && !recv_dev) return fail(SRH_E_INVALID, "null receive buffer on the root");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if (const char *e = rccl_gather_f64(c->comm, c->comm_ranks, c->comm_rank, root, v.depth, (double *)recv_dev,
	                                    (size_t)v.w*v.h, c->stream))
		return comm_failed(c, "gather", e);
	// the collective is ON the stream now; its completion is waited for here, with the bound -- a peer that dies inside it
	// must not leave this rank in a later, unbounded hipStreamSynchronize
	if (const char *e = rccl_wait_stream(c->comm, c->stream, "the depth-map gather")) return comm_failed(c, "gather", e);
	return SRH_OK;
}

extern "C" int srh_comm_allgather_depth(srh_context *c, int slot, void *recv_dev) {
	int rc = check_slot(c, slot, true); if (rc) return rc;
	if (!c->comm) return fail(SRH_E_INVALID, "srh_comm_init has not been called");
	if (!recv_dev) return fail(SRH_E_INVALID, "null receive buffer");
	HIP_TRY(hipSetDevice(c->device));
	const ViewHost &v = c->views[slot];
	if (const char *e = rccl_allgather_f64(c->comm, v.depth, (double *)recv_dev, (size_t)v.w*v.h, c->stream))
		return comm_failed(c, "all-gather", e);
	if (const char *e = rccl_wait_stream(c->comm, c->stream, "the depth-map all-gather")) return comm_failed(c, "all-gather", e);
	return SRH_OK;
}

extern "C" int srh_comm_allgather_host(srh_context *c, const double *send_host, size_t count, double *recv_host) {
	if (!c || !send_host || !recv_host || count == 0) return fail(SRH_E_INVALID, "null argument");
	if (!c->comm) return fail(SRH_E_INVALID, "srh_comm_init has not been called");
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	// the staging below is the band scratch, which a queued MultiViewStereo estimate (slot 0) still reads its support
	// windows from on its own stream: finish the estimates in flight first, like every other entry point
	if ((rc = mvs_settle_all(c))) return rc;
	// staging in the band scratch (free between runs): [send | recv]
	if ((rc = c->mem.band.wbuf.ensure(count*(size_t)(c->comm_ranks + 1)))) return rc;
	HIP_TRY(hipMemcpyAsync(c->mem.band.wbuf, send_host, count*sizeof(double), hipMemcpyHostToDevice, c->stream));
	if (const char *e = rccl_allgather_f64(c->comm, c->mem.band.wbuf, c->mem.band.wbuf + count, count, c->stream))
		return comm_failed(c, "all-gather", e);
	HIP_TRY(hipMemcpyAsync(recv_host, c->mem.band.wbuf + count, count*(size_t)c->comm_ranks*sizeof(double), hipMemcpyDeviceToHost, c->stream));
	if (const char *e = rccl_wait_stream(c->comm, c->stream, "the all-gather")) return comm_failed(c, "all-gather", e);   // (bounded: never a bare hipStreamSynchronize behind a collective)
	return SRH_OK;
}

extern "C" int srh_comm_allgather_views(srh_context *c, const int32_t *slots, int nviews) {
	int rc;
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (!c->comm) return fail(SRH_E_INVALID, "srh_comm_init has not been called");
	if (!slots || nviews < 1 || nviews > SRH_MAX_VIEWS) return fail(SRH_E_INVALID, "bad view list");
	size_t npix = 0;
	for (int v = 0; v < nviews; ++v) {
		if ((rc = check_slot(c, slots[v], true))) return rc;
		npix = std::max(npix, (size_t)c->views[slots[v]].w*c->views[slots[v]].h);
	}
	HIP_TRY(hipSetDevice(c->device));
	const int world = c->comm_ranks, rank = c->comm_rank;
	const int per = (nviews + world - 1)/world;                   // equal contributions: short ranks pad with NaN maps
	auto shard = [&](int r, int &lo, int &hi) { const int base = nviews/world, extra = nviews % world;
	                                            lo = r*base + std::min(r, extra); hi = lo + base + (r < extra ? 1 : 0); };
	// [send | recv] in the band scratch (free between runs); everything below is ordered on the context's stream
	if ((rc = c->mem.band.wbuf.ensure((size_t)(world + 1)*per*npix))) return rc;
	double *send = c->mem.band.wbuf, *recv = c->mem.band.wbuf + (size_t)per*npix;
	launch_fill(c->stream, send, (size_t)per*npix, __builtin_nan(""));
	int lo, hi;
	shard(rank, lo, hi);
	for (int v = lo; v < hi; ++v) {
		const ViewHost &vh = c->views[slots[v]];
		HIP_TRY(hipMemcpyAsync(send + (size_t)(v - lo)*npix, vh.depth, (size_t)vh.w*vh.h*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
	}
	if (const char *e = rccl_allgather_f64(c->comm, send, recv, (size_t)per*npix, c->stream))
		return comm_failed(c, "all-gather", e);
	for (int r = 0; r < world; ++r) {
		if (r == rank) continue;
		int rlo, rhi;
		shard(r, rlo, rhi);
		for (int v = rlo; v < rhi; ++v) {
			const ViewHost &vh = c->views[slots[v]];
			HIP_TRY(hipMemcpyAsync(vh.depth, recv + ((size_t)r*per + (v - rlo))*npix, (size_t)vh.w*vh.h*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
		}
	}
	if (const char *e = rccl_wait_stream(c->comm, c->stream, "the views' all-gather")) return comm_failed(c, "all-gather", e);
	return SRH_OK;
}

extern "C" int srh_comm_destroy(srh_context *c) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	if (c->comm) {
		const char *e = rccl_comm_destroy(c->comm);
		c->comm = nullptr; c->comm_ranks = 0;
		if (e) return fail(SRH_E_DEVICE, "RCCL: the communicator did not finalize: %s", e);
	}
	return SRH_OK;
}

// ------------------------------------------------------------------ measurement
extern "C" int srh_get_stats(srh_context *c, srh_stats *out) {
	if (!c || !out) return fail(SRH_E_INVALID, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	int rc = mvs_settle_all(c);
	if (rc) return rc;
	rc = fetch_counters(c, c->main_lane(), c->stats.used_dense_path);
	if (rc) return rc;
	c->stats.band_budget_bytes = (int64_t)c->budget_used;
	*out = c->stats;
	return SRH_OK;
}

extern "C" int srh_profile_enable(srh_context *c, int on) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	c->profiling = on != 0;
	return SRH_OK;
}

extern "C" int srh_profile_reset(srh_context *c) {
	if (!c) return fail(SRH_E_INVALID, "null context");
	HIP_TRY(hipSetDevice(c->device));
	int rc = drain_profile(c); if (rc) return rc;
	c->prof.clear();
	return SRH_OK;
}

extern "C" int srh_profile_get(srh_context *c, const char *name, double *total_ms, int64_t *launches) {
	if (!c || !name) return fail(SRH_E_INVALID, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	int rc = drain_profile(c); if (rc) return rc;
	auto it = c->prof.find(name);
	if (it == c->prof.end()) return fail(SRH_E_INVALID, "kernel '%s' was never launched under profiling", name);
	if (total_ms) *total_ms = it->second.ms;
	if (launches) *launches = it->second.n;
	return SRH_OK;
}

extern "C" int srh_profile_dump(srh_context *c, char *buf, size_t cap) {
	if (!c || !buf || cap == 0) return fail(SRH_E_INVALID, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	int rc = drain_profile(c); if (rc) return rc;
	size_t off = 0;
	buf[0] = 0;
	for (auto &kv : c->prof) {
		int n = snprintf(buf + off, cap - off, "%s %.6f %lld\n", kv.first.c_str(), kv.second.ms, (long long)kv.second.n);
		if (n < 0 || (size_t)n >= cap - off) break;
		off += (size_t)n;
	}
	return SRH_OK;
}
