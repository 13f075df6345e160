// srh_internal.hpp -- shared between the C-ABI host layer (srh_api.hip) and the
// gfx950 kernels (srh_kernels.hip, srh_mvs.hip, srh_dense.hip, ...).  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stereo_recon_hip.h"
#include "srh_wta.hpp"
#include "srh_stripframe.hpp"

namespace srh {

// One view as the kernels see it (device pointers).  HBM layout, all row-major:
//   rgba    u32  R | G<<8 | B<<16 | A<<24           4 B/pixel  (weights: colour distances)
//   mask    u8   1 <=> mask.pixel == WHITE           1 B/pixel  (curve candidates, reference pixels)
//   gray    f64  toGray(pixel)                       8 B/pixel  (MVS taps: pixel(), every in-bounds pixel)
//   gray_tv f64  toGray where the TwoView tap test   8 B/pixel  (mask WHITE && sample() valid:
//                passes, NaN elsewhere                           x+1<w && y+1<h)
//   depth   f64  result map                          8 B/pixel
//   census  u64  9x7 census signature of `gray`      8 B/pixel  (option "cost" = SRH_COST_CENSUS; null until a census
//                                                                run asks for it: census_kernel)
struct ViewDev {
	int32_t w, h;
	const uint32_t *rgba;
	const uint8_t  *mask;
	const double   *gray;
	const double   *gray_tv;
	double         *depth;
	srh_camera      cam;
	const uint64_t *census;
};

// Support-window buffer of one row band: tile-major, a tile = SRH_WTILE consecutive
// pixels of one image row holding T taps: wbuf[tile][tap][SRH_WTILE] (31 KB contiguous
// per tile at r=5).  A pixel's window is  base + tap*SRH_WTILE.
#define SRH_WTILE 32
__host__ __device__ inline size_t wbuf_doubles(int W, int nrows, int T) {
	return (size_t)nrows*((W + SRH_WTILE - 1)/SRH_WTILE)*SRH_WTILE*T;
}
__host__ __device__ inline size_t wbuf_offset(int W, int T, int band_row, int x) {
	const size_t tile = (size_t)band_row*((W + SRH_WTILE - 1)/SRH_WTILE) + x/SRH_WTILE;
	return tile*(size_t)T*SRH_WTILE + (x % SRH_WTILE);
}

// ---- the strip kernel's inputs (srh_strip.hip) ------------------------------------------------------------
// Window buffer, layout B ("LDS image"): wbuf[tile][row][pixel 0..31][WP], WP = taps per row padded to an even
// count -- exactly the bytes the strip kernel keeps in LDS, so a tile moves global -> LDS as one linear
// LDS-DMA copy (global_load_lds_dwordx4 writes lane-linear destinations only), and the 32 pixels' taps of one
// window row are 3 KB of contiguous bytes for the weights kernel's stores.  Tap (row, col) of a pixel is
// base + row*wimg_row_stride(R) + col; the pad tap is never read.
__host__ __device__ inline int wimg_wp(int R) { return ((2*R + 1) + 1) & ~1; }
__host__ __device__ inline int wimg_row_stride(int R) { return SRH_WTILE*wimg_wp(R); }
__host__ __device__ inline size_t wimg_doubles(int W, int nrows, int R) {
	return (size_t)nrows*((W + SRH_WTILE - 1)/SRH_WTILE)*SRH_WTILE*(size_t)((2*R + 1)*wimg_wp(R));
}
__host__ __device__ inline size_t wimg_offset(int W, int R, int band_row, int x) {
	const size_t tile = (size_t)band_row*((W + SRH_WTILE - 1)/SRH_WTILE) + x/SRH_WTILE;
	return tile*SRH_WTILE*(size_t)((2*R + 1)*wimg_wp(R)) + (size_t)(x % SRH_WTILE)*wimg_wp(R);
}
// The NaN-bordered planes the strip kernels stage from (SRH_PADL / SRH_PADR / SRH_PADY, padded_stride, padded_size) and
// PixRange, a pixel's candidate column range: srh_stripframe.hpp (host-clean: the CPU suite compiles it)

// ---- certified fused arithmetic (option "arith" = 3): CertBound, cert_bound(), cert_sure, cert_pixel_exact and the scans'
// doubt tests live in srh_wta.hpp (host-clean: the CPU suite compiles it), with the derivation; DESIGN.md section 2b

// the finish of a one-pass candidate (onepass_finish) and what a cost kernel stores for a fast-form candidate: srh_block.hpp

// ---- by-products of the winner-take-all scan (option "wta_outputs") ------------------------------------------
// Two int32 pairs per pixel of the reference view, planes back to back in one allocation: win_xy[npix][2] -- the candidate
// pixel of the other view that held minCost at the end of the scan -- then runner_xy[npix][2] -- the one that held it
// immediately before the last improvement (its cost is secondBest); (-1, -1) = none.  Every scan kernel takes the planes as
// `wout` (nullptr: the WTA = false instantiation, the code the kernels had before) and writes a pixel's pairs where it
// writes the pixel's depth.
#ifdef __HIPCC__
__device__ __forceinline__ void wta_store(int32_t *__restrict__ wout, size_t npix, size_t pv, int wx, int wy, int rx, int ry) {
	*reinterpret_cast<int2 *>(wout + 2*pv) = make_int2(wx, wy);
	*reinterpret_cast<int2 *>(wout + 2*(npix + pv)) = make_int2(rx, ry);
}
#endif
// exact costs of the two pairs (srh_wta_out.hip): min_cost[npix] and second_cost[npix] of rows [y0, y0 + nrows), in the
// reference's arithmetic (tv_cost_of under cost kind `kind`: the bits of pair_costs_kernel), from the band's window buffer in either layout
void launch_twoview_winner_costs(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int kind,
                                 int y0, int nrows, const double *wbuf, bool wimg, const int32_t *wout,
                                 double *min_cost, double *second_cost);

// Work counters accumulated by the kernels (device memory, zeroed per run).
struct Counters {
	unsigned long long n_pixels;
	unsigned long long n_eval;
	unsigned long long n_eval_device;
	unsigned long long not_row_aligned;   // pixels whose curve leaves their own row
	unsigned long long n_listed, n_slots; // row-run lists: distinct candidates / cost slots (8-column blocks) they occupy
	unsigned long long strip_overflow;    // strip kernel: tiles whose candidate range does not fit one LDS chunk
	unsigned long long n_certified, n_flagged;   // certified scan: reference pixels scanned on fused costs / flagged for the exact redo
	unsigned long long cert_overflow;     // certified redo: a flagged pixel with more candidates than the wave rescan holds (the pass is repeated in mode 0)
	unsigned long long scan_tiles_template, scan_tiles_walked;   // dense TwoView scan: 64-pixel tiles settled by the template scan / left to the per-pixel walk
	unsigned long long scan_tiles_bound;  // of scan_tiles_template: settled by the per-pixel bound (no label-by-label verification)
	unsigned long long mvs_waves_staged, mvs_waves_listed;   // MultiViewStereo walk kernel: waves (with candidates) left to the staged / the gathering cost kernel
	unsigned int strip_ticket, strip_ticket_border;   // strip kernel: work-item counters of the current launch (main, border instantiation)
	unsigned long long dbg_cycles, dbg_blocks, dbg_total_cycles, dbg_waves;   // SRH_DENSE_DBG=2 instrumentation
	unsigned long long dbg_phase[8];
	unsigned long long dbg_wave[64];      // diagnostic build: phase k of wave w of a workgroup at [8*k + w]
	unsigned long long dbg_redo[6];       // diagnostic build: twoview_redo_kernel's phase clocks (srh_dense.hip)
};

// Neighbour views of one MultiViewStereo estimate, passed to the kernels by value
// (NUM_NEIGHBOURING_VIEWS is 3 in the reference, multiviewstereo.cpp:97; srh_params.num_neighbours is a
// run-time parameter here, up to SRH_MAX_NEIGH).
#define SRH_MAX_NEIGH 8
struct NeighList { int32_t n[SRH_MAX_NEIGH]; };
inline NeighList make_neigh_list(const int32_t *neigh, int nneigh) {
	NeighList l;
	for (int i = 0; i < SRH_MAX_NEIGH; ++i) l.n[i] = (i < nneigh) ? neigh[i] : 0;
	return l;
}

// Per-pixel result of the curve-extent pass (dense path planning)
struct Extent { int32_t xmin, xmax; };

// ---- launch wrappers (srh_kernels.hip / srh_dense.hip; launch_mvs_*: srh_mvs.hip); all asynchronous on `st` ----
void launch_prep_view(hipStream_t st, const uint32_t *rgba, const uint8_t *mask, int w, int h,
                      double *gray, double *gray_tv);
void launch_fill(hipStream_t st, double *p, size_t n, double v);
// doubles per pixel of `pconst`: meanL, totalWeight, sum2, [3] 0 / 1/totalWeight, [4] SA = sum of fma(w_t, l_t, -meanL) (the
// one-pass form's sum1 = Q - m*SA; FUSED terms: an unfused w*l - meanL carries an absolute error u*|w*l| per tap, which at a
// small sum2 is beyond the certificate's bound), [5] pad (rows of 48 bytes: every tile's piece starts 16-byte aligned)
#define SRH_PC 6
// pconst (optional): SRH_PC doubles per pixel of the band -- meanL, totalWeight, sum2, all-taps-usable (0, or 1/totalWeight), SA -- the per-pixel
// constants of the dense cost kernel's fast form, computed while the window is at hand
void launch_weights(hipStream_t st, const ViewDev *views, int ref, int width, const srh_params &P,
                    int y0, int nrows, double *wbuf, size_t wstride, double *pconst = nullptr, bool wimg = false);
void launch_twoview_generic(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                            int y0, int nrows, const double *wbuf, size_t wstride, Counters *cnt, int kind = SRH_COST_NCC,
                            int32_t *wout = nullptr);
void launch_twoview_cross_check(hipStream_t st, const ViewDev *views, int self, int other, int w, int h,
                                const srh_params &P);
void launch_mvs_generic(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                        const srh_params &P, int y0, int nrows, const double *wbuf, size_t wstride,
                        double *peaks, Counters *cnt);
void launch_mvs_cross_check(hipStream_t st, const ViewDev *views, const int32_t *slots_dev, int nviews,
                            int view_index, int w, int h, const srh_params &P);

// Dense (row-aligned) TwoView path, srh_dense.hip
void launch_edge_planes(hipStream_t st, const uint32_t *rgba, int w, int h, double *edges);
// the dense TwoView path's windows kernel with its tiles by LDS-DMA (r = 5; srh_dense.hip): the padded planes it reads
void launch_geo_exp_probe(hipStream_t st, const double *x, int n, double *kout, double *lout);   // srh_debug_exp
size_t geo5_doubles(int w, int h);
void launch_geo5_planes(hipStream_t st, const double *edges, const double *gray_tv, const uint8_t *mask, int w, int h, double *out);
bool launch_geodesic_dma(hipStream_t st, const ViewDev *views, int ref, int width, const double *geo5, const srh_params &P,
                         int y0, int nrows, double *wbuf, double *pconst, int num_cus);
bool launch_geodesic_reg(hipStream_t st, const ViewDev *views, int ref, int width, const double *edges,
                         const srh_params &P, int y0, int nrows, double *wbuf, size_t wstride, double *pconst = nullptr,
                         bool wimg = false);
bool launch_adaptive_reg(hipStream_t st, const ViewDev *views, int ref, int width, const srh_params &P, int y0, int nrows,
                         double *wbuf, size_t wstride, double *pconst = nullptr, bool wimg = false);
void launch_label_plane_table(hipStream_t st, const ViewDev *views, int ref, const srh_params &P, bool mvs, double *tdist);
void launch_pinhole_label_table(hipStream_t st, const ViewDev *views, int ref, const srh_params &P, bool mvs, double *tnum);
bool launch_twoview_dense_cost_f32(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                   int y0, int nrows, const double *wbuf, size_t wstride,
                                   const double *tnum, double *cost, int cstride, Counters *cnt, const double *pconst, int form = 0);   // form 1: one-pass sums
bool launch_twoview_dense_cost(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                               int y0, int nrows, const double *wbuf, size_t wstride,
                               const double *tnum, double *cost, int cstride, Counters *cnt, const double *pconst, int arith = 0,
                               const PixRange *prange = nullptr);   // the pixels' column ranges from pixel_range_kernel (else worked out per tile)
// cflag == nullptr: the exact scan (cnt == nullptr: without counting).  cflag, nlist < 0: the certified scan on fused
// costs, flagged pixels into cflag = [count | band pixel indices].  cflag, nlist >= 0: the exact scan of the listed pixels
// (launch sized for nlist pixels, the count itself is read on the device)
void launch_twoview_scan(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                         int y0, int nrows, const double *tnum, const double *cost, int cstride,
                         Counters *cnt, const PixRange *prange, uint32_t *cflag = nullptr, int nlist = -1,
                         const double *pexact = nullptr,    // certified scan: the band's pconst when the cost kernel applies cert_pixel_exact
                         const void *tpl = nullptr, uint32_t *tilelist = nullptr,   // template scan (launch_scan_template) + the tiles it leaves: [count | tile indices]
                         int num_cus = 256, int32_t *wout = nullptr,
                         int tscan_bound = 1);              // template scan: the per-pixel bound before the label-by-label verification
// the pass's candidate template (twoview_template_kernel) into `tpl` (scan_template_bytes() bytes)
size_t scan_template_bytes();
void launch_scan_template(hipStream_t st, const ViewDev *views, int ref, int oth, const srh_params &P, int y0, int nrows,
                          const double *tnum, void *tpl);
// the cost rows of the flagged pixels in the reference's arithmetic; `cap` workgroups (the count is read on the device;
// a count above cap is reported in Counters::cert_overflow); wimg: LDS-image windows, else tile-major
bool launch_twoview_refill(hipStream_t st, int width, const srh_params &P, int y0, const PixRange *prange, const uint32_t *cflag, int cap,
                           const double *wbuf, bool wimg, const double *ref_tvp, const double *oth_tvp, double *cost, int cstride, Counters *cnt);
// refill + exact rescan of the flagged pixels in one kernel (twoview_redo_kernel: the columns beside the walk), a fixed grid of
// 512 workgroups (RD_GRID) over the list; false (nothing launched): not eligible, the caller launches the pair
bool twoview_redo_takes(const srh_params &P, int cstride);
bool launch_twoview_redo(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int y0,
                         const double *tnum, const double *wbuf, bool wimg, const double *ref_tvp, const double *oth_tvp,
                         double *cost, int cstride, const PixRange *prange, const uint32_t *cflag, int cap, Counters *cnt, int32_t *wout);
// columns the cost kernel leaves out (dense_cover_hi with `lanes` block lanes per pixel), filled in before the scan:
// a fixed small grid over filllist = [count | band pixel indices], pixel_range_kernel's list for the same form
void launch_twoview_lazy_fill(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                              int y0, int nrows, const PixRange *prange, const uint32_t *filllist, const double *wbuf, size_t wstride,
                              const double *ref_tvp, const double *oth_tvp,      // NaN-bordered planes (radius 5 / 2), else null
                              bool wimg,                                         // LDS-image windows (strip path), else tile-major
                              int lanes, bool padded,                            // the cost kernel's form: block lanes per pixel, blocks on even columns
                              double *cost, int cstride, Counters *cnt);

// Persistent strip form of the dense cost kernel, srh_strip.hip
void launch_padded_plane(hipStream_t st, const double *gray_tv, int w, int h, double *out);
void launch_padded_full(hipStream_t st, const double *gray_tv, int w, int h, int R, uint8_t *out);
void launch_pixel_range(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                        int y0, int nrows, const double *tnum, int cstride, PixRange *prange,
                        int lanes = 8, bool padded = true,     // the cost kernel's form, as launch_twoview_lazy_fill gets it
                        uint32_t *filllist = nullptr);         // [count (cleared by the caller) | pixels with left-out columns]; null: no list
int  strip_chunk_columns();
int  strip_block_lanes(int cstride, int form);
bool launch_twoview_strip_cost(hipStream_t st, const ViewDev *views, int ref, int oth, int width, int height,
                               const srh_params &P, int y0, int nrows, const double *wimg, const double *pconst,
                               const PixRange *prange, const double *ref_tvp, const double *oth_tvp,
                               const uint8_t *oth_fullp, double *cost, int cstride, Counters *cnt, int arith, int num_cus,
                               int lanes, bool raw = false);   // raw (diagnostics): certified forms without the in-kernel exact redo

#ifdef SRH_PROFILE_PHASES
void geodesic_phases_fetch(unsigned long long out[8]);
#endif
#ifdef SRH_EXPERIMENT
void exp_set(int repeat, int lds_pad);
void exp_set_scan(int mode);
void exp_set_walk(int mode);
void exp_set_rows(int mode);
#endif

// Fused row-aligned TwoView kernel (geometry + cost + WTA per 16-pixel tile), srh_fused.hip.
// SRH_FUSED_MAXC: cost-row columns (and labels) a pixel may have in LDS.
#define SRH_FUSED_MAXC 256
bool launch_twoview_fused(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                          int y0, int nrows, const double *wbuf, const double *tnum, Counters *cnt, int32_t *wout = nullptr);

// Candidate-list TwoView path for arbitrary geometry, srh_list.hip
void launch_twoview_count(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                          int y0, int nrows, int32_t *count, Counters *cnt, int *max_count, const double *tdist);
void launch_twoview_list(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                         int y0, int nrows, uint32_t *cand, int cmax, int32_t *count, Counters *cnt, int *max_count,
                         const double *tdist);
void launch_full_window(hipStream_t st, const double *gray_tv, int w, int h, int R, uint8_t *full, uint32_t *stat = nullptr);   // stat[2] (zeroed): usable centres, full windows
inline size_t full_stat_offset(size_t npix) { return (npix + 15) & ~(size_t)15; }   // the two counters live behind the map, 16-byte aligned
bool launch_twoview_list_cost(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                              int y0, int nrows, const double *wbuf, const uint8_t *full_oth,
                              const int32_t *count, const uint32_t *cand, double *cost, int cmax, Counters *cnt);
void launch_twoview_list_scan(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                              int y0, int nrows, const int32_t *count, const uint32_t *cand, const double *cost, int cmax,
                              int32_t *wout = nullptr);
// act / nact: the band's masked-in pixels (y*w + x) in the view's serpentine order -- the units of the launch, 128 per
// block and link, so that every wave is full and its 64 pixels lie side by side (also across a row change).
// wdesc / nwin (or null): per wave of the walk launch (2 per 128-pixel block and link), the windows of list slots whose
// box of the other view fits the LDS (mvs_staged_cost_kernel); mvs_staging_shape gives the buffer sizes
void mvs_staging_shape(int *maxw, size_t *desc_words_per_wave);
void launch_mvs_walk(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                     const srh_params &P, int y0, int nrows, const double *tnum, uint32_t *cand, int cmax, int32_t *count,
                     Counters *cnt, int *max_count, uint32_t *wdesc, int32_t *nwin, const uint32_t *act, int nact, bool peaks,
                     bool fast_pinhole = false);   // every neighbour a plain pinhole camera: certified label projections (with tnum)
// cert: the certified fused form (no top-K request): fused sweeps, the unit's winner certified against the bound, its
// cost recomputed in the reference's arithmetic; ambiguous units redone exactly
void launch_mvs_staged_cost(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                            const srh_params &P, int y0, int nrows, const double *wbuf, size_t wstride,
                            const uint32_t *cand, int cmax, const int32_t *count, double *best,
                            const uint32_t *wdesc, const int32_t *nwin, Counters *cnt, const uint32_t *act, int nact,
                            double *unit_peaks, bool cert = false);
void launch_mvs_list_cost(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh, int nneigh, int width,
                          const srh_params &P, int y0, int nrows, const double *wbuf, size_t wstride,
                          const uint32_t *cand, int cmax, const int32_t *count, double *best,
                          double *unit_peaks, bool peaks, const int32_t *nwin, const uint32_t *act, int nact);
void launch_mvs_combine(hipStream_t st, const ViewDev *views, int ref, int nneigh, int width, const srh_params &P,
                        int y0, int nrows, const double *best, const double *unit_peaks, double *peaks);
// hole filling (srh_filter.hip); cnt: 4 counters, see srh_filter_info
void launch_filter_gaps(hipStream_t st, const double *D, double *G, int w, int h, int gap, unsigned long long *cnt);
void launch_filter_holes(hipStream_t st, const uint8_t *mask, double *D, int w, int h, bool median, uint32_t *holes,
                         unsigned long long *cnt);
void launch_filter_median(hipStream_t st, const ViewDev *views, int slot, const srh_params &P, const double *G,
                          const uint32_t *holes, int nholes, double *D, unsigned long long *cnt);
// speckle filter (srh_speckle.hip); A, B: int32 planes of w*h; cnt: 5 counters, see srh_speckle_info
void launch_speckle_tiles(hipStream_t st, const uint8_t *mask, const double *D, int w, int h, double max_diff, int32_t *A);
void launch_speckle_merge(hipStream_t st, const double *D, int w, int h, double max_diff, int32_t *A);
void launch_speckle_flatten(hipStream_t st, const int32_t *A, size_t n, int32_t *B);
void launch_speckle_count(hipStream_t st, const int32_t *B, size_t n, int32_t *size);
void launch_speckle_apply(hipStream_t st, const int32_t *B, const int32_t *size, size_t n, int min_size, double reject, double *D,
                          unsigned long long *cnt);
// rectification (srh_rectify.hip).  The warp of slot `src` onto rect_cam, out_w x out_h: the map uv (2 doubles
// per pixel, or null) and the warped rgba + mask (both, or both null).  The way back: slot dst's depth map (w x h) from
// slot rect's, index (w*h, or null) = the rectified pixel every pixel read
void launch_rectify_warp(hipStream_t st, const ViewDev *views, int src, const srh_camera &rect_cam, int out_w, int out_h, double s,
                         double *uv, uint32_t *rgba, uint8_t *mask);
void launch_unrectify(hipStream_t st, const ViewDev *views, int rect_slot, int dst_slot, int w, int h, double s, int32_t *index);
// weighted SAD, TwoViewStereo::cost_sad (srh_sad.hip)
// full (w*h bytes): 1 where the whole (2R+1)^2 window of cost_sad's OTHER-view side is usable (inside the image, mask WHITE)
void launch_sad_full_window(hipStream_t st, const uint8_t *mask, int w, int h, int R, uint8_t *full);
// the row-run lists' cost slots (srh_rows.hip layout) with cost_sad; the windows in the LDS-image layout
bool launch_twoview_rows_sad(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                             int y0, int nrows, const double *wbuf, const uint8_t *full_sad_oth,
                             const uint32_t *rowinfo, const int32_t *meta, double *cost, int smax, Counters *cnt);
// the list-order costs (srh_list.hip layout) with cost_sad; the windows tile-major
void launch_twoview_list_sad(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                             int y0, int nrows, const double *wbuf, const int32_t *count, const uint32_t *cand,
                             double *cost, int cmax, Counters *cnt);
// cost_sad on the row-aligned dense plan (srh_sad_strip.hip; option "sad_dense"): the other view's masked gray plane and
// its cost_sad "window fully usable" bytes (launch_sad_full_window's) on the padded raster of padded_size(w, h), then the
// persistent kernel that fills every column [lo, hi] of the band's cost rows (tile-transposed, as twoview_scan_kernel reads)
void launch_padded_gray(hipStream_t st, const double *gray, const uint8_t *mask, int w, int h, double *out);
void launch_padded_bytes(hipStream_t st, const uint8_t *in, int w, int h, uint8_t *out);
bool launch_twoview_strip_sad(hipStream_t st, int width, int height, const srh_params &P, int y0, int nrows,
                              const double *wimg, const PixRange *prange, const double *ref_tvp, const double *oth_grayp,
                              const uint8_t *oth_fullp, double *cost, int cstride, Counters *cnt, int num_cus);
// cost of arbitrary pairs xy[4k..4k+3] = (x1, y1, x2, y2), the window of (x1, y1) built per lane; kind: SRH_COST_*
void launch_pair_costs(hipStream_t st, const ViewDev *views, int ref, int oth, const srh_params &P, int kind, int n,
                       const int32_t *xy, double *out);
// support-weighted census, option "cost" = SRH_COST_CENSUS (srh_census.hip)
// the 9x7 signature plane of a w x h gray plane
void launch_census(hipStream_t st, const double *gray, int w, int h, uint64_t *out);
// the row-run lists' cost slots (srh_rows.hip layout); windows in the LDS-image layout, full_oth: launch_sad_full_window's plane
bool launch_twoview_rows_census(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                int y0, int nrows, const double *wbuf, const uint8_t *full_oth,
                                const uint32_t *rowinfo, const int32_t *meta, double *cost, int smax, Counters *cnt);
// the list-order costs (srh_list.hip layout); the windows tile-major
void launch_twoview_list_census(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                int y0, int nrows, const double *wbuf, const int32_t *count, const uint32_t *cand,
                                double *cost, int cmax, Counters *cnt);
// the census cost on the row-aligned dense plan (srh_census_strip.hip; option "census_dense"): a view's signatures on the
// padded raster of padded_size(w, h) as the other side's taps (unusable behind the mask) and as the reference side's
// (unusable where gray_tv is NaN), then the persistent kernel that fills every column [lo, hi] of the band's cost rows;
// oth_fullp: launch_padded_bytes' copy of launch_sad_full_window's plane
void launch_padded_census(hipStream_t st, const uint64_t *census, const uint8_t *mask, const double *gray_tv, int w, int h,
                          uint64_t *out_other, uint64_t *out_ref);
bool launch_twoview_strip_census(hipStream_t st, int width, int height, const srh_params &P, int y0, int nrows,
                                 const double *wimg, const PixRange *prange, const uint64_t *ref_cenp, const uint64_t *oth_cenp,
                                 const uint8_t *oth_fullp, double *cost, int cstride, Counters *cnt, int num_cus);
void launch_point_cloud(hipStream_t st, const ViewDev *views, int slot, int w, int h, const srh_params &P,
                        double *xyz, uint8_t *rgb, uint8_t *valid, unsigned long long *counts);
// depth-map fusion (srh_fuse.hip).  Per entry of the slot list: its point map (3 doubles per pixel, from
// point_cloud_kernel), the "has a point" bytes and the "claimed by an earlier entry" bytes.
struct FuseViewDev { const double *pts; const uint8_t *valid; uint8_t *claimed; };
// one point per element: the staging planes of a view (indexed by pixel) and the compacted result
struct FuseCloud { double *xyz, *nrm; int32_t *src; uint8_t *rgb, *nviews, *flags; };
#define SRH_FUSE_BLOCK 256
// counters: [0] points, [1] claimed, [2] unsupported, [3] normals, [4] running total of emitted points (the scan's base)
// entry `vi` of the list: every pixel's decision (emit[pixel] = 1: a point goes out) and the point into `stage`, the
// emitted pixels of every block of SRH_FUSE_BLOCK into block_counts; flags of later entries are claimed
void launch_fuse_view(hipStream_t st, const ViewDev *views, const int32_t *slots_dev, int nviews, int vi, int w, int h,
                      const srh_params &P, double thr, double gap, int min_views, const FuseViewDev *fv,
                      uint8_t *emit, FuseCloud stage, uint32_t *block_counts, unsigned long long *counters);
// exclusive scan of the block counts on top of counters[4], which then moves on by their sum
void launch_fuse_scan(hipStream_t st, const uint32_t *block_counts, int nblocks, unsigned long long *block_offs,
                      unsigned long long *counters);
// the emitted pixels of every block to block_offs[block] + their rank in the block (wave64 ballots), in pixel order
void launch_fuse_scatter(hipStream_t st, int vi, size_t npix, const uint8_t *emit, FuseCloud stage,
                         const unsigned long long *block_offs, FuseCloud out, unsigned long long cap);
// MRF stage (srh_mrf.hip): one scratch buffer, carved the same way by every launch
struct MrfLayout {
	double *pz, *D, *Mh, *Mv, *partial, *energy;
	unsigned long long *hand; size_t hand_words;
	unsigned *status, *sync;
	int32_t *ans;
	int nparts, nbands;
	size_t sync_words, total_doubles;
};
size_t mrf_scratch_doubles(int w, int h);
void launch_mrf_layout(double *buf, int w, int h, MrfLayout &lay);
hipError_t launch_mrf_setup(hipStream_t st, double *buf, int w, int h, int K, double beta, double lambda, double phiu,
                            const double *peaks, MrfLayout &lay);
hipError_t launch_mrf_sweep(hipStream_t st, double *buf, int w, int h, int K, double psiu, int sweep);
hipError_t launch_mrf_energy(hipStream_t st, double *buf, int w, int h, int K, double psiu);
hipError_t launch_mrf_depth(hipStream_t st, const ViewDev *views, int slot, double *buf, int w, int h, int K);
// the same data, energy and depth kernels on a caller's own blocks (rows of 16 doubles per pixel), for a stage with a layout of its own
hipError_t launch_mrf_data(hipStream_t st, size_t n, int K, double beta, double lambda, double phiu, const double *peaks, double *D, double *pz);
hipError_t launch_mrf_labels_energy(hipStream_t st, int w, int h, int K, double psiu, const double *D, const double *pz, const int32_t *ans,
                                    double *partial, int nparts, double *energy);
hipError_t launch_mrf_labels_depth(hipStream_t st, const ViewDev *views, int slot, int K, const double *pz, const int32_t *ans, size_t n);
// semi-global aggregation over MultiViewStereo's peak labels (srh_mvs_sgm.hip): peak depths, data costs and sums (rows of 16
// doubles per pixel), the energy's partials and the labels in one scratch buffer of its own
struct MvsSgmLayout {
	double *pz, *D, *S, *partial, *energy;
	int32_t *ans;
	int nparts;
	size_t total_doubles;
};
size_t mvs_sgm_scratch_doubles(int w, int h);
void mvs_sgm_layout(double *buf, int w, int h, MvsSgmLayout &lay);
hipError_t launch_mvs_sgm_setup(hipStream_t st, double *buf, int w, int h, int K, double beta, double lambda, double phiu, const double *peaks);
hipError_t launch_mvs_sgm_path(hipStream_t st, double *buf, int w, int h, int K, double psiu, int k, bool first);
hipError_t launch_mvs_sgm_readoff(hipStream_t st, const ViewDev *views, int slot, double *buf, int w, int h, int K);
hipError_t launch_mvs_sgm_energy(hipStream_t st, double *buf, int w, int h, int K, double psiu);
// MRF stage of TwoViewStereo (srh_twoview_mrf.hip): the message planes, hand-over granules, labels and control words in one
// scratch buffer carved the same way by every launch; the data costs ([pixel][L] doubles) are a buffer of their own
struct TvMrfLayout {
	double *Mh, *Mv, *trash, *partial, *energy;
	unsigned long long *hand; size_t hand_words;
	unsigned *status, *sync;
	int32_t *ans;
	int nparts, nbands;
	size_t sync_words, total_doubles;
};
size_t twoview_mrf_scratch_doubles(int w, int h, int L);
void launch_twoview_mrf_layout(double *buf, int w, int h, int L, TvMrfLayout &lay);
hipError_t launch_twoview_mrf_setup(hipStream_t st, double *buf, int w, int h, int L, TvMrfLayout &lay);
hipError_t launch_twoview_mrf_sweep(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax, int sweep);
hipError_t launch_twoview_mrf_energy(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax);
hipError_t launch_twoview_mrf_depth(hipStream_t st, const ViewDev *views, int slot, const srh_params &P, double *buf, int w, int h, int L);
hipError_t launch_twoview_labels_energy(hipStream_t st, const double *costs, const int32_t *ans, double *partial, int nparts, double *energy,
                                        int w, int h, int L, double lambda, double smax);
// semi-global aggregation over the label cost volume (srh_twoview_sgm.hip): the sums S, the energy's partials and the labels
// in one scratch buffer; the data costs ([pixel][L] doubles) are a buffer of their own
struct TvSgmLayout {
	double *S, *partial, *energy;
	int32_t *ans;
	int nparts;
	size_t total_doubles;
};
size_t twoview_sgm_scratch_doubles(int w, int h, int L);
void twoview_sgm_layout(double *buf, int w, int h, int L, TvSgmLayout &lay);
hipError_t launch_twoview_sgm_path(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax, int k, bool first);
hipError_t launch_twoview_sgm_readoff(hipStream_t st, const ViewDev *views, int slot, const srh_params &P, double *buf, int w, int h, int L);
hipError_t launch_twoview_sgm_energy(hipStream_t st, double *buf, const double *costs, int w, int h, int L, double lambda, double smax);
// the label cost volume of rows [y0, y0 + nrows): cost [pixel][label], pixel (optional) [pixel][label][x2, y2]
hipError_t launch_twoview_label_costs(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int kind,
                                      int y0, int nrows, double fill, double *cost, int32_t *pixel);
void launch_epipolar_preview(hipStream_t st, const ViewDev *views, int ref, int oth, double zmin, double zmax, int nd,
                             int nq, const double *xy, double *out, int32_t *counts);
void launch_refraction_error(hipStream_t st, const ViewDev *views, int v1, int v2, int n, const double *p1, const double *p2, double *err);
void launch_epipolar_curves(hipStream_t st, const ViewDev *views, int ref, int oth, const srh_params &P, int mvs,
                            int nq, const int32_t *xy, int32_t *out, int cap, int32_t *counts);

// run-blocked candidate lists, srh_rows.hip
#define SRH_ROWS_NR 32
void launch_twoview_rows_list(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                              int y0, int nrows, uint32_t *cand, int cmax, int32_t *count, uint32_t *rowinfo,
                              int32_t *meta, int smax, Counters *cnt, int *maxes, const double *tdist);
// arith: 0 = the reference's arithmetic, 3 = certified fused sweeps (values stored for the certified scan)
bool launch_twoview_rows_cost(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                              int y0, int nrows, const double *wbuf, const uint8_t *full_oth,
                              const uint32_t *rowinfo, const int32_t *meta, double *cost, int smax, Counters *cnt, int arith = 0,
                              const double *pconst = nullptr,    // pconst: the band's per-pixel constants from the weights kernel (else made in the kernel)
                              const double *oth_tvp = nullptr, int num_cus = 256, const uint32_t *full_stat = nullptr);  // the other view's NaN-bordered plane: masked fast blocks + single candidates (else: a block is fast when all 8 are)
// cflag == nullptr: exact scan.  cflag, nlist < 0: certified scan (flags into cflag = [count | band pixel indices]).
// cflag, nlist >= 0: the exact scan of the listed pixels (after launch_twoview_rows_refill)
void launch_twoview_rows_scan(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                              int y0, int nrows, const int32_t *count, const uint32_t *cand, int cmax,
                              const uint32_t *rowinfo, const int32_t *meta, const double *cost, int smax,
                              uint32_t *cflag = nullptr, int nlist = -1, Counters *cnt = nullptr, int32_t *wout = nullptr);
bool launch_twoview_rows_refill(hipStream_t st, int width, int oth_width, const srh_params &P, int y0,
                                const uint32_t *cflag, int cap, const double *wbuf, const double *ref_tvp, const double *oth_tvp,
                                const uint32_t *rowinfo, const int32_t *meta, double *cost, int smax, Counters *cnt);
// image scaling in Qt's arithmetic, srh_scale.hip
int  scale_target_size(int sw, int sh, double scale, int mode, int *dw, int *dh, const char **why);   // SRH_OK, or the refusal's code
bool scale_axis_inside(int s, int d);                   // every run of the smooth scale ends inside the axis
bool scale_fast_maps(int sw, int sh, int dw, int dh, bool has_alpha, int32_t *map);   // dw source columns, then dh source rows
void launch_premultiply(hipStream_t st, uint32_t *px, size_t n, bool has_alpha);      // in place; an opaque source: alpha := 255
// src: 16-byte aligned and readable up to 3 pixels past its end
void launch_smooth_scale(hipStream_t st, const uint32_t *src, int sw, int sh, uint32_t *dst, int dw, int dh);
void launch_fast_scale(hipStream_t st, const uint32_t *src, int sw, uint32_t *dst, int dw, int dh, const int32_t *map, bool has_alpha);
void launch_scale_mask(hipStream_t st, const uint32_t *img, int mw, int mh, bool alpha_only, uint8_t *mask, int w, int h);
// RCCL exchange, srh_comm.hip (functions return nullptr or an error string)
const char *rccl_unique_id_get(void *out128);
const char *rccl_comm_init(void **comm, int nranks, int rank, const void *id128);
const char *rccl_comm_destroy(void *comm);   // finalize (non-blocking communicator) + destroy, bounded; error text or null
bool rccl_available();                        // librccl can be loaded and has the entry points (else: SRH_E_UNSUPPORTED)
// bounded wait for everything `st` holds (a collective included): event + ncclCommGetAsyncError polled to the timeout
const char *rccl_wait_stream(void *comm, hipStream_t st, const char *what);
void rccl_comm_abort(void *comm);
void rccl_set_timeout_ms(int ms);      // how long a call into RCCL may stay "in progress" (rendezvous, collectives); default 120 s
int  rccl_version();                   // NCCL_VERSION_CODE of the loaded librccl, 0 if there is none
const char *rccl_gather_f64(void *comm, int nranks, int rank, int root, const double *send, double *recv,
                            size_t count, hipStream_t st);
const char *rccl_allgather_f64(void *comm, const double *send, double *recv, size_t count, hipStream_t st);

} // namespace srh
