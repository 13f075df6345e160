/*
 * stereo_recon_hip.h -- C-ABI of libstereo_recon_hip.so: the MI355X (gfx950) dense
 * matching-cost / support-weight aggregation / winner-take-all path of
 * StereoReconstruction, i.e. what the reference computes inside
 *   TwoViewStereo::computeCostVolumes / crossCheck   (stereo/twoviewstereo.cpp:233-502, 596-672)
 *   MultiViewStereo::computeInitialEstimate / crossCheck (stereo/multiviewstereo.cpp:524-662, 666-729)
 * and the helpers they call.
 *
 * Plain C: opaque context, POD structs, caller-owned buffers, integer status
 * codes, no exceptions, no torch / Qt / Eigen types.  A Qt adapter (or the
 * Qt-free C++ classes in stereoreconstruction_amd/host/) sits on top and keeps
 * the reference's TwoViewStereo / MultiViewStereo class API; INTEGRATION.md shows
 * the binding.  All arithmetic on the path is IEEE double, evaluated in the
 * reference's operation order with FMA contraction off.
 *
 * Every entry point returns SRH_OK (0) or a negative SRH_E_* code;
 * srh_last_error() returns a human-readable message for the calling thread.
 */
#ifndef STEREO_RECON_HIP_H
#define STEREO_RECON_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRH_ABI_VERSION 5

enum {
	SRH_OK = 0,
	SRH_E_INVALID = -1,    /* bad argument (NULL, size mismatch, slot out of range ...) */
	SRH_E_DEVICE = -2,     /* HIP runtime error (message has the hipError string) */
	SRH_E_NO_DEVICE = -3,  /* no usable GPU: the library has NO CPU fallback */
	SRH_E_CANCELLED = -4,  /* cancel flag observed between launches */
	SRH_E_UNSUPPORTED = -5
};

enum { SRH_WEIGHT_ADAPTIVE = 0, SRH_WEIGHT_GEODESIC = 1 };
enum { SRH_MAX_VIEWS = 64 };
/* The largest width and the largest height of a view.  srh_view_upload and srh_view_upload_scaled (by the scaled size)
 * refuse anything larger with SRH_E_UNSUPPORTED before they allocate or launch, and leave the slot as it was.  It is the
 * smallest per-kernel limit of DESIGN.md 4h (the row-run lists keep columns and row origins as 16-bit signed numbers):
 * whatever upload accepts, every path computes what the reference computes. */
#define SRH_MAX_VIEW_DIM 32767

/* Snapshot of a reference `Camera` (project/camera.hpp:168-185): the adapter
 * copies these at TwoViewStereo construction / MultiViewStereo::initialize so the
 * GUI may keep mutating its Camera objects (races).
 * 3x3 matrices are row-major. */
typedef struct srh_camera {
	double K[9], Kinv[9], R[9], Rinv[9];
	double t[3], C[3];
	double dist[5];          /* k1,k2,p1,p2,k3 -- LensDistortions order (project.cpp:143-147) */
	int32_t is_distorted;    /* Camera::isDistorted() */
	int32_t is_refractive;   /* Camera::isRefractive() */
	double plane_normal[3];  /* Camera::plane().normal(), camera-local, unit */
	double plane_dist;       /* Camera::plane().distance() */
	double refr_index;       /* Camera::refractiveIndex() */
	double pdir[3];          /* Camera::principleRay().direction() */
} srh_camera;

/* Every constant the reference hard-codes on this path, with its default
 * (twoviewstereo.cpp:64-80, multiviewstereo.cpp:90-102, adaptiveweight.cpp:26,
 * geodesicweight.cpp:33-41) plus the run-time arguments of
 * TwoViewStereo::TwoViewStereo / MultiViewStereo::initialize. */
typedef struct srh_params {
	double  min_depth, max_depth;
	int32_t num_depth_levels;
	int32_t window_radius;        /* TwoView 5, MVS 2 */
	double  image_scale;          /* images handed over are ALREADY scaled by this */
	int32_t weight_kind;          /* SRH_WEIGHT_* ; reference default geodesic */
	int32_t geodesic_iters;       /* 3 */
	double  geodesic_sigma;       /* 50 */
	double  geodesic_init;        /* 1e6 */
	double  adaptive_color_sigma; /* 10 */
	double  weight_cutoff;        /* 1e-10 */
	double  bad_ret;              /* 1000 */
	double  max_color_diff;       /* 120 */
	double  second_best_factor;   /* 0.95 */
	double  wta_margin;           /* 1e-10 (the reference's constant; a negative value is honoured by visiting every curve point: slow paths) */
	double  inconsistency_thresh; /* 1 */
	double  peak_threshold;       /* 0.95 */
	double  cross_check_threshold;
	double  neighbour_min_dot;    /* 0.2 */
	int32_t top_k;                /* 9 */
	int32_t num_neighbours;       /* 3 */
} srh_params;

/* Counters of the last run on a context (for N_eval reporting). */
typedef struct srh_stats {
	int64_t n_pixels;        /* reference pixels with mask == WHITE */
	int64_t n_eval;          /* cost evaluations the reference would have performed */
	int64_t n_eval_device;   /* cost evaluations actually performed on the device */
	int32_t used_dense_path; /* 1 if the row-aligned dense kernels ran */
	int32_t used_fused_kernel; /* 1 if that was the single fused kernel (cost rows never leave the CU) */
	int32_t used_strip_kernel; /* 1 if the cost kernel was the persistent strip form (srh_strip.hip) */
	int32_t band_retries;    /* runs repeated with thinner row bands after a band buffer did not fit (since srh_create) */
	/* certified arithmetic (option "arith" = 3), last TwoView pass: reference pixels scanned on fused costs, and those of
	 * them whose decisions the error bound did not cover and that were re-evaluated in the reference's arithmetic */
	int64_t n_certified;
	int64_t n_flagged;
	int64_t band_budget_bytes;  /* band budget the last run worked with (requested, capped by free device memory) */
	/* last MultiViewStereo estimate on the list path: 64-pixel waves (per neighbour) whose candidate windows were
	 * evaluated from LDS copies of the other view (mvs_staged_cost_kernel) / by gathers (mvs_list_cost_kernel: a window
	 * over an image border, too large, too many) */
	int64_t mvs_waves_staged, mvs_waves_listed;
	/* last TwoView pass on the dense path: 64-pixel tiles whose pixels all verified the pass's candidate template and were
	 * scanned over it (twoview_tscan_kernel) / tiles left to the per-pixel curve walk (twoview_scan_kernel) */
	int64_t scan_tiles_template, scan_tiles_walked;
	/* of scan_tiles_template: tiles whose pixels were all settled by the per-pixel bound (option "tscan_bound", DESIGN.md
	 * 2d), without the label-by-label verification */
	int64_t scan_tiles_bound;
} srh_stats;

typedef struct srh_context srh_context;

/* Progress / cancellation hooks = Task::progressUpdate / stageUpdate / isCancelled
 * (gui/task.hpp:57-105).  `cancel` is polled between kernel launches. */
typedef void (*srh_progress_fn)(int step, const char *stage, void *user);

/* ---- library ---- */
int         srh_abi_version(void);
/* 16 hex digits: hash of the library's sources at build time (which build produced a measurement) */
const char *srh_build_id(void);
const char *srh_last_error(void);
int         srh_device_count(int *count);
/* Hardware queues the HIP runtime was asked for (GPU_MAX_HW_QUEUES in the process environment, else the runtime's
 * default of 4).  srh_mvs_mrf_estimate_views keeps one stream per view busy: with 16 queues the MRF stage of 8 views
 * takes 150 ms, with the default 4 queues 277 ms (profiles/r02_mrf_views.txt).  The variable is read when HIP
 * initialises, so the HOST APPLICATION sets it before its first HIP call; this library never alters the environment. */
int         srh_hw_queues_requested(void);

/* ---- parameters and cameras (host-side math only) ---- */
void srh_params_twoview_defaults(srh_params *p);   /* twoviewstereo.cpp:64-80 */
void srh_params_mvs_defaults(srh_params *p);       /* multiviewstereo.cpp:90-102 */
/* Camera::set(K,R,t) + setLensDistortion + setPlane/setRefractiveIndex
 * (project/camera.cpp:225-240, 302-344).  dist / plane_normal may be NULL. */
int  srh_camera_from_krt(const double K[9], const double R[9], const double t[3],
                         const double dist[5],
                         const double plane_normal[3], double plane_dist, double refr_index,
                         srh_camera *out);
/* Camera::setP (project/camera.cpp:251-288, the path project files take: project.cpp:118-135): P is the
 * row-major 3x4 projection matrix; it is scaled by 1/|P[2,0:3]|^2, its left 3x3 block RQ-factorised
 * (Householder QR of the row-reversed transpose, as Eigen's HouseholderQR does it) into K (positive
 * diagonal) and R, t = K^-1 P[:,3]; then as srh_camera_from_krt. */
int  srh_camera_from_p(const double P[12], const double dist[5],
                       const double plane_normal[3], double plane_dist, double refr_index,
                       srh_camera *out);
/* The certified arithmetic's error bound (option "arith" = 3) for these parameters, host arithmetic only:
 * a fast-form candidate with A = sqrt(sum2), B = sqrt(sum3) has |cost_fused - cost_reference| <= k1/B + k2/A + k3, and is
 * certified when that is <= e0, i.e. sum3 >= srh_cert_sigma3(p, mvs, sum2); the one-pass form also needs
 * Q3 <= zmax2*sum3.  m_hi = max_color_diff + e0; ok = 0: the parameters leave the bound no room (the reference's
 * arithmetic runs).  mvs != 0: the free cost_ncc of MultiViewStereo (score itself, e0 = 2^-36). */
typedef struct srh_cert_info {
	double e0, k1, k2, k3, zmax2, m_hi;
	int32_t ok, taps;
} srh_cert_info;
int    srh_cert_bound(const srh_params *p, int mvs, srh_cert_info *out);
double srh_cert_sigma3(const srh_params *p, int mvs, double sum2);
/* The template scan's per-pixel bound (option "tscan_bound"), host arithmetic only, for pixel (x, y) of the
 * reference view against the template pixel (tx, ty) (the scan takes the middle of the view's row band):
 * |x2(x, y, d) - x2(tx, ty, d) - (x - tx)| <= E for every label d, x2 the reference's projection of label d into the other
 * view; eU / eU_template: the bound of either pixel's fast form against the reference's arithmetic; dyU: any two labels'
 * y2 differ by at most that; room_col / room_one / room_proj: the smallest room of the template pixel's column, one-pixel
 * and projectability decisions; pixel_ok / template_ok: the pixel's / the template's own conditions hold; passes: the
 * pixel's candidate list is certainly the template's. */
typedef struct srh_tscan_bound_info {
	double E, eU, eU_template, dyU;
	double room_col, room_one, room_proj;
	int32_t pixel_ok, template_ok, passes, pad_;
} srh_tscan_bound_info;
int    srh_tscan_bound(const srh_camera *refcam, const srh_camera *othcam, const srh_params *p,
                       int tx, int ty, int x, int y, srh_tscan_bound_info *out);
/* MultiViewStereo::runTask neighbour selection (multiviewstereo.cpp:335-360):
 * neigh[v*p->num_neighbours + k], count[v]. */
int  srh_mvs_neighbours(int nviews, const srh_camera *cams, const srh_params *p,
                        int32_t *neigh, int32_t *count);

/* ---- context ---- */
int  srh_create(int device_ordinal, srh_context **out);
void srh_destroy(srh_context *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL = the context's own. */
int  srh_set_stream(srh_context *ctx, void *hip_stream);
int  srh_set_hooks(srh_context *ctx, const volatile int *cancel, srh_progress_fn progress, void *user);
int  srh_synchronize(srh_context *ctx);
/* TwoView matching cost (option "cost"): TwoViewStereo::cost_ncc (default), cost_sad (twoviewstereo.cpp:864-905), or the
 * support-weighted census cost, which the reference does not have.  The value 2 is not a cost. */
enum { SRH_COST_NCC = 0, SRH_COST_SAD = 1, SRH_COST_CENSUS = 3 };
/* By-products of the TwoView winner-take-all scan a pass keeps per reference pixel (option "wta_outputs") */
enum { SRH_WTA_WINNERS = 1, SRH_WTA_COSTS = 2 };
/* Tuning / test switches (results never depend on them, "arith" = 1 / 2, "cost", "filter_invalid" and "speckle_*" excepted):
 *   "force_generic"   0 default paths; 1 never the dense row-aligned TwoView kernels nor the MVS list kernels;
 *                     2 additionally no candidate lists at all (one thread per pixel walks and costs its curve)
 *   "fused"           1: row-aligned pairs run the single fused kernel (geometry + cost + WTA per 16-pixel tile
 *                     in LDS: no cost rows or candidate lists in device memory); 0 (default): the three-kernel form
 *                     (cost rows staged in device memory, separate scan), which is the faster one on MI355X today
 *   "arith"           3 (default) CERTIFIED: the strip kernel's cost loops run with fused multiply-adds (half the FP64
 *                     instructions), the WTA scan checks every comparison it makes against a proven bound on the
 *                     difference between fused and reference costs, and the pixels with a comparison inside the bound
 *                     (srh_stats.n_flagged of n_certified) are re-evaluated in the reference's arithmetic: depth maps
 *                     are the same bits as mode 0 (tests/test_gpu_arith_modes.py).  Kernels without a
 *                     fused form run the reference's arithmetic.  0: the reference's arithmetic everywhere, operation
 *                     by operation.  1: opt-in "fma" -- fused cost loops, UNCHECKED; a winner can change between
 *                     near-tied candidates (rate measured by bench.py --arith fma).  2: opt-in "f32" -- the dense cost
 *                     loops in single precision, two candidates per packed instruction (srh_dense_f32.hip); costs agree
 *                     with the reference's to ~6 digits (rate measured by bench.py --arith f32).  MODES 1 AND 2 ARE THE
 *                     ONLY OPTION VALUES THAT CHANGE RESULTS; row-aligned TwoView path only.
 *   "force_dense"     1: the row-aligned dense plan is proposed for every undistorted, non-refractive pair,
 *                     not only for rigs the host check accepts (the device verifies every candidate and the
 *                     run is repeated on the general kernels when one leaves its row: a test hook for that path)
 *   "strip"           1 (default): the dense cost kernel runs in its persistent strip form (one workgroup walks a
 *                     tile column down the rows, every input enters LDS by LDS-DMA); 0: one workgroup per tile;
 *                     4 / 8: force the 4-wave / 8-wave form of the strip kernel.  Results are identical bits.
 *                     SRH_WEIGHT_GEODESIC with geodesic_sigma <= 0 (weights that are not finite outside the image) takes
 *                     one workgroup per tile whatever the option says.
 *   "mvs_staged"      1 (default): the MultiViewStereo list cost kernel takes its 25-tap windows from LDS copies of the
 *                     other view (one box per stretch of list slots and wave) where they fit; 0: every window is gathered
 *                     from memory (round 2's kernel).  Results are identical bits.
 *   "mvs_async"       1 (default): srh_mvs_initial_estimate only queues a view's kernels, on one of two side streams in
 *                     turn (two views in flight); 0: one view at a time, the call returns when the view is done.
 *                     Either way the maps are complete whenever another entry point can observe them.
 *   "tv_overlap"      1 (default): srh_twoview_compute queues its second pass on a stream and band buffers of its own beside
 *                     the first (the passes share only the views; the cross-check waits for both); 0: one after the other
 *                     on the context's stream.  Identical bits; the second set of band buffers counts against the budget.
 *   "tscan"           1 (default): on the dense path the scan makes the candidate sequence once per pass and every pixel verifies
 *                     its own curve against it (template scan; a tile with a pixel that does not verify is walked per pixel);
 *                     0: every tile by the per-pixel curve walk.  Identical bits (srh_stats.scan_tiles_template / _walked).
 *   "tscan_bound"     1 (default): the template scan settles a pixel by ONE error bound for all its labels, held against
 *                     the room the template pixel found in its own decisions (srh_tscan_bound is the same arithmetic on the
 *                     host); a tile with a pixel the bound does not settle is verified label by label.  0: every tile label
 *                     by label.  Identical bits (srh_stats.scan_tiles_bound).
 *   "geodma"          1 (default): on the dense path (GeodesicWeight, radius 5) the support windows come from the persistent
 *                     kernel that fetches its tiles by LDS-DMA from a second copy of the view's edge / tap / mask planes with
 *                     their borders written out (made on first use after an upload: 42 bytes per pixel of device memory; no
 *                     room for it: the other kernel runs); 0: the register-staged windows kernel.  Identical bits.
 *   "side_weights"    1 (default): the row-run path computes a band's support windows on a side stream beside its list kernel;
 *                     0: behind it on the pass's own stream (profiling: every kernel's own duration).  Identical bits.
 *   "list_rows"       1 (default) candidate lists are costed in row runs; 0 in list order
 *   "band_budget_mb"  device scratch per row band the caller asks for (default 32768: a 1920x1080x256 refractive pair
 *                     in one band).  A run never plans with more than a quarter of the device memory that is free at
 *                     that moment (hipMemGetInfo), and a run whose band buffers still do not fit is repeated with the
 *                     budget halved (srh_stats.band_retries) instead of failing: results do not depend on the split.
 *   "mem_limit_mb"    pretend the device has at most this much memory to give (0 = off; tests of the above)
 *   "debug_alloc_limit_mb"  refuse band buffers above this size as if the device were out of memory (0 = off; tests)
 *   "debug_mvs_cmax_hint"   the list capacity the next MultiViewStereo estimate is queued with (0 = forget; test of the redo of a
 *                     view whose lists were cut)
 *   "cost"            CHANGES RESULTS.  SRH_COST_NCC (0, default): the weighted NCC of cost_ncc.  SRH_COST_SAD (1): the
 *                     support-weighted, truncated SAD of cost_sad (min(|gl - gr|, max_color_diff) per tap, the left tap
 *                     sample() and the right tap pixel() behind both masks; bad_ret for numPixels <= 4 or totalWeight <=
 *                     1e-10), the WTA, ratio test and cross-check unchanged.  SAD runs in the reference's arithmetic;
 *                     "arith" does not apply to it.  By default it runs on the candidate lists, rectified rigs too; with
 *                     "sad_dense" = 1 a rectified rig takes the dense plan, its cost rows filled by the persistent SAD
 *                     strip kernel (there is no per-tile and no fused SAD kernel).  srh_twoview_cost_rows under SAD needs
 *                     "sad_dense" = 1 (else SRH_E_UNSUPPORTED).  SRH_COST_CENSUS (3; not in the reference): cost_sad's tap
 *                     rule, totalWeight, numPixels and bad_ret rule with the per-tap term replaced by the Hamming distance
 *                     of the two pixels' census signatures (srh_view_census), sum = fma(weight, distance, sum); the result
 *                     is sum / totalWeight, a value in [0, 62]; max_color_diff is not read.  The WTA, ratio test,
 *                     cross-check, filters, label cost volume, "wta_outputs" and "subpixel" run unchanged on it.  By
 *                     default census runs on the candidate lists (row runs, list order) and the walk kernel only
 *                     (srh_stats.used_dense_path is 0) and srh_twoview_cost_rows returns SRH_E_UNSUPPORTED; with
 *                     "census_dense" = 1 a rectified rig takes the dense plan, its cost rows filled by the persistent
 *                     census strip kernel (there is no per-tile and no fused census kernel).  "arith" and "sad_dense" do
 *                     not apply to it.  Any other value: SRH_E_INVALID.
 *   "sad_dense"       0 (default): cost_sad on the candidate lists.  1: under "cost" = SRH_COST_SAD a pair that is row-aligned
 *                     (the rig test of the NCC dense plan), with window radius 5 or 2, "force_generic" off and a candidate
 *                     range that fits the strip kernel's chunk (cstride + 32 <= 320 columns) takes the row-aligned dense
 *                     plan: twoview_strip_sad_kernel fills the cost rows (every column of every pixel's range, for every
 *                     image size and band), the NCC plan's range, template and scan kernels run unchanged behind it,
 *                     uncertified.  srh_stats.used_dense_path and used_strip_kernel are then 1.  Any other pair -- a rig
 *                     that is not row-aligned, another radius, a wider range, a plan the device refutes (a range wider
 *                     than the chunk after all, a candidate off its row, "force_dense" included) -- runs on the row-run,
 *                     list-order or walk kernels exactly as with 0.  The fused plan is never taken under SAD.  Nothing
 *                     changes under "cost" = SRH_COST_NCC.  Identical bits: a tuning switch like "strip" and "tscan".
 *   "census_dense"    0 (default): the census cost on the candidate lists.  1: under "cost" = SRH_COST_CENSUS a pair that
 *                     meets "sad_dense"'s conditions (row-aligned rig, window radius 5 or 2, "force_generic" off, cstride + 32
 *                     <= 320 columns) takes the row-aligned dense plan: twoview_strip_census_kernel fills the cost rows
 *                     (every column of every pixel's range), the range, template and scan kernels run unchanged behind it,
 *                     uncertified; srh_stats.used_dense_path and used_strip_kernel are then 1.  Any other pair, and a plan
 *                     the device refutes, runs on the row-run, list-order or walk kernels exactly as with 0.  Nothing
 *                     changes under the other costs.  Identical bits: a tuning switch.
 *   "wta_outputs"     never changes a depth map.  0 (default): a WTA pass keeps the depth only -- no allocation, no extra store.
 *                     SRH_WTA_WINNERS (1): every pass ref -> oth (srh_twoview_wta, both passes of srh_twoview_compute) also keeps,
 *                     per reference pixel, win_xy -- the candidate pixel of `oth` that held minCost at the end of the scan -- and
 *                     runner_xy -- the one that held it immediately before the last improvement, whose cost is the secondBest of
 *                     the ratio test; (-1, -1) = none.  SRH_WTA_WINNERS | SRH_WTA_COSTS (3): also min_cost and second_cost, the
 *                     cost of (x, y) -> win_xy / runner_xy in the reference's arithmetic whatever "arith" chose the winner -- the
 *                     bits srh_twoview_pair_costs returns for that pair under the current "cost"; +INF = none.  2 alone:
 *                     SRH_E_INVALID.  16 / 32 bytes per pixel of the reference view in device memory, allocated by the first
 *                     pass that keeps them; read with srh_view_wta_outputs*.  They describe the WTA stage: the cross-check and
 *                     "filter_invalid" do not touch them.
 *   "subpixel"        CHANGES RESULTS.  0 (default): off -- not one extra launch, allocation or store.  1: every TwoView WTA pass
 *                     (srh_twoview_wta, both passes of srh_twoview_compute, row ranges included) refines the depth of the rows
 *                     it has decided before it returns, hence before the cross-check, the speckle filter and the hole filling:
 *                     a parabola through the reference's costs of the kept winner and of its two neighbours on the pixel's
 *                     curve -- the visited pixels at Chebyshev distance 1 from the winner whose candidate depths lie next
 *                     below and next above the winner's -- places the match between two pixels of the other view, and the
 *                     depth is triangulated there (DESIGN.md 4n has the definition).  Internally the pass keeps winners and
 *                     costs as under "wta_outputs" = 3; what srh_view_wta_outputs* show is still what "wta_outputs" asked
 *                     for.  Read with srh_view_subpixel*.  No effect on srh_twoview_compute_mrf / _sgm (no scan runs there)
 *                     and on MultiViewStereo.  Other values: SRH_E_INVALID.
 *   "mvs_subpixel_search"  how srh_mvs_view_subpixel finds a pixel's winner: 0 (default) among the curve pixels near the
 *                     projection of the pixel's point, exhaustively where that finds none; 1: exhaustively everywhere (the
 *                     same planes: the law the default is tested against).  Other values: SRH_E_INVALID.
 *   "filter_invalid"  0 (default, as the reference's call site under #if 0): srh_twoview_compute ends with the cross-check;
 *                     SRH_FILTER_* flags (1 gaps, 2 median, 3 both): it then runs srh_view_filter_invalid on both maps,
 *                     with progress steps 6 "Filling invalid pixels..." and, with the median, 7 "Filtering invalid pixels..."
 *   "filter_gap_width" the gap width srh_twoview_compute's filter uses (default 2, GAP_WIDTH_THRESHOLD)
 *   "filter_replay"   1: every median hole is selected by the exact replay of the heap (a test hook: identical bits; the
 *                     replay is today the only selection)
 *   "speckle_min_size"  CHANGES RESULTS.  0 (default): off -- not one extra launch, allocation or copy.  n > 0:
 *                     srh_twoview_compute, srh_twoview_compute_mrf and srh_twoview_compute_sgm run srh_view_filter_speckles
 *                     with min_size = n and the reject value +INF on both maps, between the cross-check and the
 *                     "filter_invalid" tail, with a stage text of its own ("Removing speckles...") at progress step 5, the
 *                     cross-check's step.  Negative values: SRH_E_INVALID.
 *   "speckle_diff_steps"  CHANGES RESULTS (under "speckle_min_size" only).  The stage's max_diff in depth steps (default 2):
 *                     max_diff = (double)steps * ((max_depth - min_depth)/(double)(num_depth_levels - 1)).  Values < 1:
 *                     SRH_E_INVALID.
 * The library reads no environment variable: what a host runs is what it set here. */
int  srh_set_option(srh_context *ctx, const char *name, long value);

/* ---- views: what VectorImage::fromQImage + the mask test hold (util/vectorimage.cpp:48-64) ----
 * rgba: w*h*4 bytes R,G,B,A of the ALREADY SCALED image; mask: w*h bytes,
 * 1 <=> mask.pixel(x,y)==WHITE, NULL = all WHITE.  Host pointers; copied.
 * w or h above SRH_MAX_VIEW_DIM: SRH_E_UNSUPPORTED, the slot keeps what it held. */
int  srh_view_upload(srh_context *ctx, int slot, int w, int h,
                     const uint8_t *rgba, const uint8_t *mask, const srh_camera *cam);
int  srh_view_size(srh_context *ctx, int slot, int *w, int *h);
/* ---- views at FILE resolution: the scaling the reference performs first, on the device ----
 * MultiViewStereo::initialize (multiviewstereo.cpp:216-241) smooth-scales every image with scaledToWidth(width*imageScale,
 * Qt::SmoothTransformation) and takes the mask from the alpha channel of a second copy scaled with Qt::FastTransformation;
 * TwoViewStereo's constructor (twoviewstereo.cpp:89-124) smooth-scales both images and both mask images.  These entry
 * points do the same in Qt 5.9.7's integer arithmetic, bit for bit, without Qt: an opt-in beside srh_view_upload, which
 * still takes ALREADY SCALED bytes.
 *   size    dw = (int)(src_w*image_scale); f = dw/src_w; SRH_SCALE_SMOOTH: dh = (int)(f*src_h + 0.9999), SRH_SCALE_FAST:
 *           dh = floor(f*src_h + 0.5) (one less than the smooth height now and then: 101x77 at 0.5 gives 50x39 and 50x38).
 *           dw <= 0 (or dh <= 0): SRH_E_INVALID.  dw == src_w: the identity (Qt returns the image itself, not
 *           premultiplied).  Anything else that is not a strict downscale in both axes: SRH_E_UNSUPPORTED.
 *   smooth  a source with alpha (has_alpha != 0: what QImage makes Format_ARGB32) is premultiplied by Qt's integer rule and
 *           the result holds premultiplied bytes, which the reference reads raw; has_alpha == 0 (Format_RGB32): the A bytes
 *           handed over are ignored and alpha is 255.
 *   fast    nearest neighbour by Qt's two placement rules (with / without alpha); with alpha a fully transparent pixel
 *           comes out as four zero bytes.
 * rgba buffers: R, G, B, A bytes, HOST memory. */
enum { SRH_SCALE_SMOOTH = 0, SRH_SCALE_FAST = 1 };
/* how srh_view_upload_scaled derives the slot's mask:
 *   SRH_MASK_NONE          every pixel WHITE
 *   SRH_MASK_ALPHA_FAST    MultiViewStereo: has_alpha != 0: WHITE <=> alpha == 255 on the fast-scaled copy of the image; rows of
 *                          the image beyond that copy's height are not WHITE (the reference's mask image is that much shorter
 *                          and VectorImage::pixel out of bounds is not WHITE).  has_alpha == 0: every pixel WHITE.
 *   SRH_MASK_IMAGE_SMOOTH  TwoViewStereo: mask_rgba (mask_w x mask_h) smooth-scaled by ITS OWN width; WHITE <=> r = g = b =
 *                          a = 255 in the scaled raw bytes, pixels beyond the scaled mask image are not WHITE.  mask_rgba ==
 *                          NULL (a null QImage): every pixel WHITE. */
enum { SRH_MASK_NONE = 0, SRH_MASK_ALPHA_FAST = 1, SRH_MASK_IMAGE_SMOOTH = 2 };
/* the size scaledToWidth gives; needs no device */
int  srh_scaled_size(int src_w, int src_h, double image_scale, int mode, int *w_out, int *h_out);
/* host -> device -> host: rgba_out receives the srh_scaled_size(...) pixels; w_out / h_out may be NULL */
int  srh_image_scale(srh_context *ctx, const uint8_t *rgba, int src_w, int src_h, int has_alpha, double image_scale, int mode,
                     uint8_t *rgba_out, int *w_out, int *h_out);
/* The view at file resolution into `slot`: scaled on the device, mask by mask_rule, then exactly what srh_view_upload does
 * with the same scaled bytes and mask -- srh_view_size reports the scaled size and every later call behaves the same.
 * mask_rgba / mask_w / mask_h / mask_has_alpha are read under SRH_MASK_IMAGE_SMOOTH only.  A refused shape (image or mask
 * image) leaves the slot as it was.  The staging buffers come from the allocator of the view planes and go back to it. */
int  srh_view_upload_scaled(srh_context *ctx, int slot, int src_w, int src_h, const uint8_t *rgba, int has_alpha,
                            const uint8_t *mask_rgba, int mask_w, int mask_h, int mask_has_alpha,
                            double image_scale, int mask_rule, const srh_camera *cam);
/* what the slot holds: rgba_out w*h*4 bytes, mask_out w*h bytes (1 = WHITE); each may be NULL; synchronous */
int  srh_view_image_download(srh_context *ctx, int slot, uint8_t *rgba_out, uint8_t *mask_out);
/* The context keeps one depth map (w*h doubles) per view slot in device memory. */
int  srh_view_depth_download(srh_context *ctx, int slot, double *host_out);
/* The census signature plane of a view, w*h words row-major to a HOST buffer: one 64-bit signature per pixel, taken from
 * toGray of every pixel (the mask is not consulted).  Bit k = (dy + 3)*9 + (dx + 4), dy in -3..3, dx in -4..4, is set iff
 * (dx, dy) != (0, 0), the neighbour (x + dx, y + dy) lies inside the image and its gray value is smaller than the centre's;
 * bits 31 and 63 are always 0.  The 9x7 size does not depend on window_radius.  Made on first use after an upload and kept
 * with the slot; what "cost" = SRH_COST_CENSUS matches on.  Synchronous. */
int  srh_view_census(srh_context *ctx, int slot, uint64_t *host_out);
int  srh_view_depth_upload(srh_context *ctx, int slot, const double *host_in);
int  srh_view_depth_device_ptr(srh_context *ctx, int slot, void **dev_ptr);
/* The by-products of the last TwoView WTA pass that had `slot` as its reference view (option "wta_outputs"):
 * win_xy, runner_xy: w*h*2 int32 (x, y), (-1, -1) = none; min_cost, second_cost: w*h doubles, +INF = none.  A pass over
 * rows [y0, y1) writes those rows only, as it does in the depth map; rows no pass has written since the planes were made
 * hold the "none" values.  srh_view_wta_outputs: host buffers, each may be NULL, synchronous (it completes what is in
 * flight first, like srh_view_depth_download).  srh_view_wta_outputs_device: the device planes themselves, with the
 * semantics of srh_view_depth_device_ptr; each argument may be NULL.  srh_view_wta_outputs_state: what the slot holds --
 * *flags = SRH_WTA_* bits, 0 when it holds nothing, *oth_slot = the other view of that pass (-1: none).
 * Both getters return SRH_E_INVALID when the slot holds nothing (the option was off, or no pass yet), when the slot was
 * uploaded again since, when the slot's depth map last came from srh_twoview_mrf* (no scan made it), and when a cost
 * plane is asked for and only the winners were kept. */
int  srh_view_wta_outputs(srh_context *ctx, int slot, int32_t *win_xy, int32_t *runner_xy, double *min_cost, double *second_cost);
int  srh_view_wta_outputs_device(srh_context *ctx, int slot, void **win_xy, void **runner_xy, void **min_cost, void **second_cost);
int  srh_view_wta_outputs_state(srh_context *ctx, int slot, int *flags, int *oth_slot);
/* What option "subpixel" did to each pixel of the last TwoView WTA pass that had `slot` as its reference view:
 *   SRH_SUBPX_NONE          no finite depth or no kept winner (NaN, +INF, outside the mask): nothing to refine
 *   SRH_SUBPX_NO_NEIGHBOUR  the curve has no visited pixel beside the winner with a smaller, or none with a larger, depth
 *   SRH_SUBPX_FLAT          D = (cm - c0) + (cp - c0) is not > 0: the three costs have no minimum between the neighbours
 *   SRH_SUBPX_OUTSIDE       |delta| = |0.5*(cm - cp)/D| is not <= 0.5: the parabola's minimum lies beyond half a step
 *   SRH_SUBPX_REFINED       the depth was triangulated at winner + |delta|*(neighbour - winner) (delta == 0: its bits kept)
 * delta: w*h doubles, 0 where the pixel is not refined; > 0 towards n+, the neighbour of larger depth.  neigh_xy: w*h*4
 * int32 (n-.x, n-.y, n+.x, n+.y), (-1, -1) = none.  cls: w*h bytes.  Rows no pass has written hold NONE, 0 and (-1, -1).
 * srh_view_subpixel: host buffers, each may be NULL, synchronous; srh_view_subpixel_device: the device planes themselves;
 * srh_view_subpixel_info: the pixels of each class in the slot's plane.  All three return SRH_E_INVALID where
 * srh_view_wta_outputs does (nothing held, uploaded since, map from the MRF / SGM stage) and when the pass ran with the
 * option off. */
enum { SRH_SUBPX_NONE = 0, SRH_SUBPX_NO_NEIGHBOUR = 1, SRH_SUBPX_FLAT = 2, SRH_SUBPX_OUTSIDE = 3, SRH_SUBPX_REFINED = 4 };
typedef struct srh_subpixel_info {
	int64_t n_class[5];          /* pixels per SRH_SUBPX_* class */
	int64_t n_moved;             /* of the REFINED ones: delta != 0 */
} srh_subpixel_info;
int  srh_view_subpixel(srh_context *ctx, int slot, double *delta, int32_t *neigh_xy, uint8_t *cls);
int  srh_view_subpixel_device(srh_context *ctx, int slot, void **delta, void **neigh_xy, void **cls);
int  srh_view_subpixel_info(srh_context *ctx, int slot, srh_subpixel_info *info);
/* Sub-pixel depth for a MultiViewStereo view, as a stage of its own on the slot's FINISHED depth map: no
 * estimator keeps the (neighbour, pixel) that gave a depth, but the map identifies it.  Per pixel of view_slot, z0 its depth:
 *   SRH_SUBPX_NONE          outside the mask, z0 not finite, or z0 <= 0 (NaN, +INF, the "no peak" value -1)
 *   the winner              the first (i, q) -- neighbours in the order of neigh_slots, q in the order of the pixel's
 *                           MultiViewStereo curve in that neighbour -- whose candidate depth equals z0 bit for bit
 *   SRH_SUBPX_NO_WINNER     there is none: the depth is no candidate depth of these neighbours
 *   n-, n+, the classes     as under option "subpixel", on the winner's curve, with the free cost_ncc of MultiViewStereo
 *                           (higher is better) of the pixel against n-, the winner and n+: classify(-c-, -c0, -c+)
 * IT REFINES WHATEVER THE SLOT HOLDS, whichever call made it -- srh_mvs_initial_estimate, _mrf, _sgm or srh_view_depth_upload
 * -- so call it once per estimate, before srh_view_filter_speckles and srh_mvs_cross_check, with the neighbour list the
 * estimate used.  A refined map identifies no winner: a second call leaves NO_WINNER nearly everywhere and changes (nearly)
 * nothing; it is idempotent only by that accident.
 * The winner is searched among the curve pixels near the projection of the pixel's point at z0 into each neighbour, and a
 * pixel with no winner there is searched exhaustively (info->n_fallback counts those); option "mvs_subpixel_search" = 1
 * searches every pixel exhaustively: the same planes, several times the work.
 * win: w*h*3 int32 per pixel -- the index into neigh_slots, then cx, cy; (-1, -1, -1) = none.  delta, neigh_xy, cls: as
 * srh_view_subpixel.  All four are HOST buffers and each may be NULL; info may be NULL.  Synchronous; whatever "mvs_async"
 * has in flight is completed first.  The support windows are computed band by band ("band_budget_mb").  nneigh 0..8.
 * SRH_E_INVALID: a slot without an image, view_slot among its neighbours, nneigh out of range.  Nothing of the stage is
 * allocated or launched unless it is called. */
enum { SRH_SUBPX_NO_WINNER = 5 };
typedef struct srh_mvs_subpixel_info {
	int64_t n_class[6];          /* pixels per SRH_SUBPX_* class, SRH_SUBPX_NO_WINNER included */
	int64_t n_moved;             /* of the REFINED ones: delta != 0 */
	int64_t n_fallback;          /* pixels the narrowed search handed to the exhaustive one (the NO_WINNER ones among them) */
} srh_mvs_subpixel_info;
int  srh_mvs_view_subpixel(srh_context *ctx, int view_slot, const int32_t *neigh_slots, int nneigh, const srh_params *p,
                           srh_mvs_subpixel_info *info, double *delta, int32_t *win, int32_t *neigh_xy, uint8_t *cls);
/* Asynchronous device-to-device copy of the slot's depth map (w*h doubles) into caller-owned
 * DEVICE memory of `dst_bytes` bytes (e.g. a tensor that RCCL then gathers); ordered on the context
 * stream.  SRH_E_INVALID when the buffer is smaller than the map (views may differ in size). */
int  srh_view_depth_copy_to_device(srh_context *ctx, int slot, void *dst_dev, size_t dst_bytes);
/* The reverse: the slot's depth map is replaced by its first w*h doubles of `src_bytes` bytes of DEVICE
 * memory (a map another rank computed, received through RCCL); asynchronous, ordered on the context
 * stream.  SRH_E_INVALID when fewer than w*h doubles are offered. */
int  srh_view_depth_copy_from_device(srh_context *ctx, int slot, const void *src_dev, size_t src_bytes);

/* ---- TwoViewStereo ----
 * One pass of computeCostVolumes (twoviewstereo.cpp:260-333 with ref=left,
 * :431-501 with ref=right): depth map of `ref_slot` against `oth_slot`, rows
 * [y0,y1) (y1<=0: all).  The result stays in the slot's device depth map.  Kernels are
 * enqueued on the context stream; the call returns after the run's verification / sizing
 * read-backs (one or two stream synchronisations), results need no further synchronisation
 * before srh_view_depth_* / srh_twoview_cross_check on the same context.
 * Three implementations produce identical bits: dense row-aligned kernels (rectified
 * pinhole rigs, radius 5 or 2), candidate-list kernels (any geometry, radius <= 5), and a
 * one-thread-per-pixel curve-walk kernel (last resort). */
int  srh_twoview_wta(srh_context *ctx, int ref_slot, int oth_slot, const srh_params *p,
                     int y0, int y1);
/* crossCheck (twoviewstereo.cpp:596-672): left pass, then right pass reading the
 * filtered left map; in place on the two slots' depth maps. */
/* DIAGNOSTIC (evidence for the certified arithmetic, tests/test_gpu_cert_rows.py): the cost rows of reference rows
 * [y0, y1) on the row-aligned dense plan as the cost kernel leaves them -- what the scan looks up.  form: 0 = the
 * reference's arithmetic, 3 = two fused sweeps, 5 = one-pass (the certified forms), 1 = fused unchecked, 2 = the
 * single-precision kernel ("arith" = 2) in the form option "f32_form" selects: always the per-tile kernel
 * (*used_strip_kernel = 0 whatever "strip" says), raw is ignored (tests/test_gpu_f32_rows.py); raw != 0: the
 * certified forms WITHOUT their in-kernel exact redo (an uncertified candidate is NaN).  Layout of cost_out (doubles):
 * [row][tile of 32 pixels][k = column - range.lo, < *cstride_out][pixel of the tile]; an entry the kernels never wrote
 * reads as a NaN with all bits set.  range_out: (lo, hi) per pixel, hi < lo = no candidates.  cost_out == NULL: only
 * *cstride_out (to size the buffer: rows * ceil(w/32)*32 * cstride doubles).  The rows must fit one band;
 * SRH_E_UNSUPPORTED when the pair does not take the dense plan.  Under "cost" = SRH_COST_SAD with "sad_dense" = 1: the
 * SAD cost rows in the same layout, *used_strip_kernel = 1; form must be 0 (else SRH_E_INVALID), raw is ignored; with
 * "sad_dense" = 0: SRH_E_UNSUPPORTED.  Under "cost" = SRH_COST_CENSUS the same with "census_dense": the census cost rows
 * with the option 1 and form 0, SRH_E_INVALID for another form, SRH_E_UNSUPPORTED with the option 0. */
int  srh_twoview_cost_rows(srh_context *ctx, int ref_slot, int other_slot, const srh_params *p, int y0, int y1, int form, int raw,
                           double *cost_out, size_t cost_doubles, int32_t *range_out, int *cstride_out, int *used_strip_kernel);
/* cost_sad (kind SRH_COST_SAD), cost_ncc (SRH_COST_NCC) or the census cost (SRH_COST_CENSUS) of n arbitrary pairs: xy holds n x (x1, y1, x2, y2), (x1, y1) a
 * pixel of ref_slot (else SRH_E_INVALID), (x2, y2) any pixel position of oth_slot (taps outside it are skipped).  The
 * support window of (x1, y1) is built on the device (p->weight_kind, p->window_radius <= 5).  Host pointers; synchronous.
 * The backend of the host classes' protected cost_sad / cost_ncc / cost_census. */
int  srh_twoview_pair_costs(srh_context *ctx, int ref_slot, int oth_slot, const srh_params *p, int kind, int n,
                            const int32_t *xy, double *out);
/* DIAGNOSTIC (tests/test_gpu_geodesic_exp.py): the GeodesicWeight kernels evaluate exp(-w/sigma) (geodesicweight.cpp:128-130)
 * by the device library's exp sequence written out in their source (srh_dense.hip, geo_exp_n: constants of THIS ROCm's
 * ocml) -- this entry evaluates n arguments by that sequence (kernel_out) and by the library's exp() itself (library_out),
 * so that a ROCm whose exp has moved shows up as a bit difference here, not as a last-bit drift of the windows. */
int  srh_debug_exp(srh_context *ctx, const double *x, int n, double *kernel_out, double *library_out);
int  srh_twoview_cross_check(srh_context *ctx, int left_slot, int right_slot, const srh_params *p);
/* computeDepthMaps minus colourisation (twoviewstereo.cpp:150-227): both passes +
 * cross-check, progress steps 1,3,5,8 (option "filter_invalid": 1,3,5,6[,7],8 and the hole filling; option "speckle_min_size": a second 5, "Removing speckles...", and the speckle filter before it); synchronous; host outputs may be NULL.  The two passes
 * run side by side on the device (option "tv_overlap"); the progress steps are emitted as the
 * passes are QUEUED. */
int  srh_twoview_compute(srh_context *ctx, int left_slot, int right_slot, const srh_params *p,
                         double *left_depth_out, double *right_depth_out);

/* ---- MultiViewStereo ----
 * computeInitialEstimate(view) non-MRF result (multiviewstereo.cpp:524-604,654-660)
 * for `view_slot` against `nneigh` neighbour slots (0..8; the reference keeps 3), rows [y0,y1).
 * peaks_dev (optional, DEVICE pointer, w*h*top_k*2 doubles) receives the sorted
 * top-K (cost,depth) pairs the MRF branch would consume.
 * With option "mvs_async" (default) and no peaks_dev the call queues the view's kernels on a side stream and returns:
 * consecutive calls overlap two views; every other entry point of the context (downloads, copies, cross-checks,
 * srh_synchronize, srh_get_stats ...) first completes what is in flight, so a caller never sees an unfinished map.
 * An error of a queued view (cancellation, device error) is reported by the call that completes it. */
int  srh_mvs_initial_estimate(srh_context *ctx, int view_slot, const int32_t *neigh_slots, int nneigh,
                              const srh_params *p, int y0, int y1, void *peaks_dev);
/* crossCheck(view) (multiviewstereo.cpp:666-729) over `nviews` slots listed in view
 * order; call for view index 0..nviews-1 in order to reproduce the reference's
 * sequential dependence. */
int  srh_mvs_cross_check(srh_context *ctx, const int32_t *slots, int nviews, int view_index,
                         const srh_params *p);

/* ---- MultiViewStereo, MRF branch ----
 * What computeInitialEstimate does with the top-K peaks when the reference is built with CONFIG+=mrf
 * (multiviewstereo.cpp:481-516 cost functions, :610-652 optimisation and label -> depth): a W x H grid, K + 1 labels
 * (the K peaks of each pixel + "unknown"), sequential TRW-S sweeps until the energy drops by no more than
 * min_energy_drop or max_iters + 1 sweeps were made, then depth = the chosen peak's depth (INF for "unknown" or a
 * placeholder peak) where the mask is WHITE.  PARITY UNPINNED: the reference takes the optimiser from a third-party
 * library (-lMRF) that is not in its tree; DESIGN.md 5 says what was restated instead. */
typedef struct srh_mrf_params {
	double  beta, lambda;         /* BETA 1, LAMBDA 1 (multiviewstereo.cpp:98-99) */
	double  phi_u, psi_u;         /* PHIU 0.5, PSIU 0.002 (:100-101) */
	int32_t max_iters;            /* 50 (:631) */
	double  min_energy_drop;      /* 5 (:641) */
} srh_mrf_params;
typedef struct srh_mrf_info {
	int32_t iterations;           /* sweeps made */
	double  energy_initial;       /* totalEnergy() of the all-zero labelling */
	double  energy_final;
} srh_mrf_info;
void srh_mrf_params_defaults(srh_mrf_params *m);
/* peaks_dev: the DEVICE buffer srh_mvs_initial_estimate filled for this view (w*h*top_k (cost, depth) pairs),
 * 1 <= top_k <= 15.  Writes the slot's depth map.  info may be NULL. */
int  srh_mvs_mrf_estimate(srh_context *ctx, int view_slot, int top_k, const void *peaks_dev,
                          const srh_mrf_params *m, srh_mrf_info *info);
/* computeInitialEstimate as a CONFIG+=mrf build runs it: srh_mvs_initial_estimate with the peaks kept in the
 * context's own scratch, then srh_mvs_mrf_estimate on them. */
int  srh_mvs_initial_estimate_mrf(srh_context *ctx, int view_slot, const int32_t *neigh_slots, int nneigh,
                                  const srh_params *p, const srh_mrf_params *m, srh_mrf_info *info);
/* The same for several views at once: srh_mvs_initial_estimate_peaks keeps a view's peaks in the context, then
 * srh_mvs_mrf_estimate_views runs the MRF stage of all listed views side by side (a sweep fills a quarter of the
 * chip and is bound by its own dependency chain; each view stops by the reference's rule for itself) and writes
 * their depth maps.  infos: nviews entries, may be NULL. */
int  srh_mvs_initial_estimate_peaks(srh_context *ctx, int view_slot, const int32_t *neigh_slots, int nneigh, const srh_params *p);
int  srh_mvs_mrf_estimate_views(srh_context *ctx, const int32_t *view_slots, int nviews, const srh_mrf_params *m, srh_mrf_info *infos);
/* State of the last srh_mvs_mrf_estimate on this context, to HOST buffers (each may be NULL): labels (w*h, what
 * getLabel(p) returns), data_costs (w*h*(top_k+1)), messages (w*h*2*(top_k+1): [pixel][towards x+1, towards y+1][label],
 * the message currently stored on that edge).  w, h, top_k say what the caller sized its buffers for: the call fails
 * with SRH_E_INVALID unless they are the dimensions of that run (srh_mvs_mrf_dims reports them).  There is no such
 * state after srh_mvs_mrf_estimate_views (every view has scratch of its own) or after the view was uploaded again. */
int  srh_mvs_mrf_dims(srh_context *ctx, int *w, int *h, int *top_k);
int  srh_mvs_mrf_state(srh_context *ctx, int w, int h, int top_k, int32_t *labels, double *data_costs, double *messages);

/* ---- TwoViewStereo, MRF stage (second half) ----
 * The step after winner-take-all: a regularised depth map from the full label cost volume.  PARITY UNPINNED: the
 * reference's branch is compile-time dead (#undef USE_MRF, twoviewstereo.cpp:35), no longer compiles against its own
 * cost_ncc signature, and hands the energy to alpha-expansion from a third-party library that is not in its tree: no
 * compiled reference can pin any of it.
 * FROM THE REFERENCE'S LINES:
 *   labels 0 .. D-1 with depthFromLabel (:981-985); a label's pixel in the other view is pointFromDepth on the pixel's
 *   ray, project into the other view (:309-313), times image_scale, truncated toward zero (the live path's rule, the int
 *   parameters at :1019-1028; huge coordinates saturate as everywhere on this path).  The dead branch's "- 0.5"
 *   (:314-315) is deliberately NOT taken: it dates from a cost_ncc that sampled at fractional positions and would select
 *   the pixel left of / above the one that contains the projection.
 *   data cost of (pixel, label) = the live path's pair cost (cost_ncc, or cost_sad under option "cost") at (x, y) and the
 *   label's pixel with the support window of (x, y); WINDOW_SIZE*BAD_RET = (2*window_radius + 1)*bad_ret (:258) where
 *   pointFromDepth or project fails and on every label of a pixel whose mask is not WHITE (never costed, :270-271).
 *   E = sum_p D_p(l_p) + sum_(p,q) lambda*min(|l_p - l_q|, smooth_max) over the 4-connected W x H grid, weight 1, every
 *   pixel a node (the graph of Expansion(width, height, ...), :347); SMOOTHNESS_EXP 1, _MAX 2, _LAMBDA 0.25 (:69-71).
 *   start: messages zero, labelling all 0 (energy_initial is its energy); loop: do { one sweep } while (prev - energy >
 *   min_energy_drop && numIters-- > 0) with 50 and 5 (:378-390); output: depthFromLabel(label) where the mask is WHITE
 *   (:324), NaN elsewhere; no ratio test and no INF from this stage; crossCheck follows unchanged.
 * OURS: the optimiser -- sequential TRW-S, the engine of the MultiViewStereo branch above (gamma = 1/2, forward sweep,
 *   backward sweep, labels read off by a forward pass, minima taken with ">" so that the lowest index wins a tie, the
 *   minimum message subtracted at every update) with L = D labels.  The reference's masked 8-neighbour graph (:351-368) is
 *   NOT restated: it indexes its pixel map out of bounds at the image border and registers every interior edge from both
 *   ends -- there is nothing well-defined to restate.
 * LIMITS: 2 <= D <= 256, smooth_exp == 1, 0 < smooth_max <= 4 (else SRH_E_UNSUPPORTED); lambda >= 0, max_iters >= 0.
 * Data costs must be finite for the results to be defined bit for bit. */
typedef struct srh_twoview_mrf_params {
	int32_t smooth_exp;           /* SMOOTHNESS_EXP 1 (twoviewstereo.cpp:69) */
	double  smooth_max, lambda;   /* SMOOTHNESS_MAX 2, SMOOTHNESS_LAMBDA 0.25 (:70-71) */
	int32_t max_iters;            /* 50 (:378) */
	double  min_energy_drop;      /* 5 (:390) */
} srh_twoview_mrf_params;
void srh_twoview_mrf_params_defaults(srh_twoview_mrf_params *m);   /* needs no device */
/* what pixel_out holds (both coordinates) for a label whose projection failed and for every label of a masked-out pixel */
#define SRH_LABEL_PIXEL_NONE (-2147483647 - 1)
/* The label cost volume of rows [y0, y1) (y1 <= 0: all) of ref_slot against oth_slot, to HOST buffers: cost_out
 * [pixel][label] doubles (rows*w*D), pixel_out (may be NULL) [pixel][label][x2, y2] the labels' pixels in the other view.
 * Every entry that is not the fill value is the bits srh_twoview_pair_costs returns for that pair and cost kind (option
 * "cost").  window_radius <= 5.  A building block and a test window; synchronous. */
int  srh_twoview_label_costs(srh_context *ctx, int ref_slot, int oth_slot, const srh_params *p, int y0, int y1,
                             double *cost_out, int32_t *pixel_out);
/* The optimiser on a caller's DEVICE volume (w*h*L doubles, [pixel][label], L == p->num_depth_levels): writes the slot's
 * depth map with the depth range of p.  The counterpart of srh_mvs_mrf_estimate.  A run needs two message planes of
 * w*h*L doubles beside the volume (+ the hand-over granules); when that does not fit the free device memory (option
 * "mem_limit_mb" honoured) the call fails with SRH_E_DEVICE and a message that names the bytes needed, before anything
 * is queued -- there are no bands: a sweep needs the whole grid.  The cancel flag is polled between sweeps.  (A volume
 * on a 16-byte boundary with L a multiple of its labels per lane, ceil(L/64), is moved 16 bytes at a time: same bits.) */
int  srh_twoview_mrf_optimize(srh_context *ctx, int view_slot, const srh_params *p, int L, const void *costs_dev,
                              const srh_twoview_mrf_params *m, srh_mrf_info *info);
/* One direction: the label cost volume in the context's scratch (three volumes in all: 12.7 GB at 1920x1080x256), the
 * optimiser, the depth map of ref_slot. */
int  srh_twoview_mrf(srh_context *ctx, int ref_slot, int oth_slot, const srh_params *p,
                     const srh_twoview_mrf_params *m, srh_mrf_info *info);
/* computeDepthMaps as a USE_MRF build runs it: both directions one after the other, then the cross-check; progress steps
 * 1, 2 "Optimizing...", 3, 4 "Optimizing...", 5, 8 (option "filter_invalid": 6 and 7 where srh_twoview_compute puts
 * them); synchronous; host outputs and infos (two entries: left, right) may be NULL. */
int  srh_twoview_compute_mrf(srh_context *ctx, int left_slot, int right_slot, const srh_params *p,
                             const srh_twoview_mrf_params *m, double *left_depth_out, double *right_depth_out,
                             srh_mrf_info *infos);
/* State of the last srh_twoview_mrf / srh_twoview_mrf_optimize on this context (the semantics of srh_mvs_mrf_state), to
 * HOST buffers (each may be NULL): labels (w*h), data_costs (w*h*L; only after srh_twoview_mrf -- the volume of
 * srh_twoview_mrf_optimize is the caller's: SRH_E_INVALID), messages (w*h*2*L: [pixel][towards x+1, towards y+1][label]).
 * After srh_twoview_compute_mrf the state is that of its second (right) direction. */
int  srh_twoview_mrf_dims(srh_context *ctx, int *w, int *h, int *L);
int  srh_twoview_mrf_state(srh_context *ctx, int w, int h, int L, int32_t *labels, double *data_costs, double *messages);

/* ---- TwoViewStereo, semi-global aggregation over the label cost volume ----
 * NOT IN THE REFERENCE.  Between the winner-take-all and TRW-S: one pass along up to 8 path directions over the volume of
 * the MRF stage, with that stage's smoothness term -- a second, non-iterative minimiser of the same energy (compare
 * srh_sgm_info.energy with srh_mrf_info.energy_final on the same volume).  No iteration, no stopping rule.
 * DEFINITION (the device reproduces it bit for bit; tests/sgm_ref.py restates it):
 *   C          the data costs [pixel][label], w*h*L finite doubles, what srh_twoview_label_costs produces; masked-out
 *              pixels are nodes and carry the fill value, as in the MRF stage.
 *   directions (dx, dy) = (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (+1,-1) (-1,+1); bit k of path_mask enables
 *              direction k (0xFF: all; 0x0F: classic 4-path SGM).
 *   per enabled direction r, pixels in path order, q = p - r:
 *              q outside the image:  L_r(p, .) = C(p, .)
 *              otherwise, with prev = L_r(q, .):
 *                g    = min_k prev[k]
 *                M[d] = min( min over integers j with |j| < smooth_max and 0 <= d+j < L of (prev[d+j] + lambda*|j|),
 *                            g + lambda*smooth_max )
 *                L_r(p, d) = C(p, d) + (M[d] - g)
 *              every + and - is one IEEE double operation, lambda*|j| and lambda*smooth_max one product each, nothing is
 *              contracted.  With smooth_max = 2 this is Hirschmueller's recurrence with P1 = lambda, P2 = 2*lambda.  (The
 *              window form above and the direct form min_k (prev[k] + lambda*min(|d - k|, smooth_max)) are the same bits.)
 *   S(p, d)    the sum of L_r(p, d) over the enabled directions in ascending k, left to right: ((L_a + L_b) + L_c) + ...
 *   label(p)   the lowest d that attains min_d S(p, d)
 *   depth(p)   depthFromLabel(label) where the mask is WHITE, NaN elsewhere; crossCheck follows unchanged; no ratio test.
 *   energy     E(label) under the MRF stage's energy (the 4-connected grid, lambda*min(|l_p - l_q|, smooth_max)).
 * LIMITS: those of srh_twoview_mrf_params with their status codes: 2 <= L <= 256, smooth_exp == 1, 0 < smooth_max <= 4
 * (else SRH_E_UNSUPPORTED); lambda >= 0; path_mask 0 or any bit above bit 7: SRH_E_INVALID. */
typedef struct srh_twoview_sgm_params {
	int32_t smooth_exp;           /* 1 */
	double  smooth_max, lambda;   /* 2, 0.25: the MRF stage's */
	int32_t path_mask;            /* 0xFF */
} srh_twoview_sgm_params;
void srh_twoview_sgm_params_defaults(srh_twoview_sgm_params *m);   /* needs no device */
typedef struct srh_sgm_info {
	int32_t paths;                /* directions aggregated (the bits set in path_mask) */
	double  energy;               /* E(label) */
} srh_sgm_info;
/* The aggregation on a caller's DEVICE volume (w*h*L doubles, [pixel][label], L == p->num_depth_levels; read only): writes
 * the slot's depth map with the depth range of p.  The counterpart of srh_twoview_mrf_optimize, with its argument checks.
 * A run needs one volume S of w*h*L doubles (+ the labels) beside the data costs; when that does not fit the free device
 * memory (option "mem_limit_mb" honoured) the call fails with SRH_E_DEVICE and a message that names the bytes needed,
 * before anything is queued, and the depth map stays untouched.  The cancel flag is polled between directions.  (Volumes
 * on a 16-byte boundary with L a multiple of an even number of labels per lane, ceil(L/64), are moved 16 bytes at a time:
 * same bits.)  info may be NULL. */
int  srh_twoview_sgm_aggregate(srh_context *ctx, int view_slot, const srh_params *p, int L, const void *costs_dev,
                               const srh_twoview_sgm_params *m, srh_sgm_info *info);
/* One direction of the pair: the label cost volume in the context's scratch (two volumes in all: 8.5 GB at 1920x1080x256),
 * the aggregation, the depth map of ref_slot. */
int  srh_twoview_sgm(srh_context *ctx, int ref_slot, int oth_slot, const srh_params *p,
                     const srh_twoview_sgm_params *m, srh_sgm_info *info);
/* Both directions one after the other, then the cross-check; progress steps 1, 2 "Aggregating...", 3, 4 "Aggregating...",
 * 5, 8 (option "filter_invalid": 6 and 7 where srh_twoview_compute_mrf puts them); option "cost" selects NCC or SAD as it
 * does there; synchronous; host outputs and infos (two entries: left, right) may be NULL. */
int  srh_twoview_compute_sgm(srh_context *ctx, int left_slot, int right_slot, const srh_params *p,
                             const srh_twoview_sgm_params *m, double *left_depth_out, double *right_depth_out,
                             srh_sgm_info *infos);
/* State of the last srh_twoview_sgm / srh_twoview_sgm_aggregate on this context (the semantics of srh_twoview_mrf_state),
 * to HOST buffers (each may be NULL): labels (w*h), data_costs (w*h*L; only after srh_twoview_sgm -- the volume of
 * srh_twoview_sgm_aggregate is the caller's: SRH_E_INVALID), sums (w*h*L: S).  Forgotten when the view is uploaded again.
 * After srh_twoview_compute_sgm the state is that of its second (right) direction. */
int  srh_twoview_sgm_dims(srh_context *ctx, int *w, int *h, int *L);
int  srh_twoview_sgm_state(srh_context *ctx, int w, int h, int L, int32_t *labels, double *data_costs, double *sums);

/* ---- MultiViewStereo, semi-global aggregation over the top-K peak labels ----
 * NOT IN THE REFERENCE.  The step between "best peak wins" and the MRF branch: one pass along up to 8 path directions over
 * the label space and the energy of the MRF branch above -- a second, non-iterative minimiser of that energy (compare
 * srh_sgm_info.energy with srh_mrf_info.energy_final on the same peaks).  No iteration, no stopping rule, no host round
 * trips between directions.
 * DEFINITION (the device reproduces it bit for bit; tests/mvs_sgm_ref.py restates it):
 *   labels     0 .. K-1 are the pixel's peaks as srh_mvs_initial_estimate writes them (sorted ascending, (0, -1) as
 *              placeholders), K is "unknown"; 1 <= K = top_k <= 15 as in the MRF branch, with its status codes.  Every pixel
 *              is a node, masked-out pixels included, as in the MRF branch.
 *   D(p, l)    the MRF branch's dataCost, by its kernel: lambda*exp(-beta*cost) for a peak, lambda for a placeholder
 *              (depth < 0), phi_u for "unknown" -- the bits srh_mvs_mrf_state reports after an MRF run on the same peaks.
 *   V(q, k; p, d)  the MRF branch's smoothnessCost between label k of pixel q and label d of pixel p: 0 when both are
 *              "unknown", psi_u when exactly one is, 2*psi_u when both are peaks and either depth is < 0, otherwise
 *              2.0*fabs(zq - zp)/(zq + zp): one subtraction, one addition, one product and one IEEE division, nothing
 *              contracted.
 *   directions (dx, dy) = (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,-1) (+1,-1) (-1,+1), the order of srh_twoview_sgm_params;
 *              bit k of path_mask enables direction k.
 *   per enabled direction r, pixels in path order, q = p - r:
 *              q outside the image:  L_r(p, .) = D(p, .)
 *              otherwise, with prev = L_r(q, .):
 *                g    = min_k prev[k]
 *                M[d] = min over k = 0 .. K of (prev[k] + V(q, k; p, d))
 *                L_r(p, d) = D(p, d) + (M[d] - g)
 *              every + and - is one IEEE double operation.
 *   S(p, d)    the sum of L_r(p, d) over the enabled directions in ascending k, left to right: ((L_a + L_b) + L_c) + ...
 *   label(p)   the lowest d that attains min_d S(p, d)
 *   depth(p)   the MRF branch's rule: where the mask is WHITE the chosen peak's depth if label < K and that depth is > 0,
 *              else +INF; untouched elsewhere.  srh_mvs_cross_check follows unchanged.
 *   energy     totalEnergy() of the labels under the MRF branch's energy (its kernels): comparable with
 *              srh_mrf_info.energy_final on the same peaks.
 * PRECONDITIONS: lambda, phi_u, psi_u >= 0 and beta finite, else SRH_E_INVALID; path_mask 0 or any bit above bit 7:
 * SRH_E_INVALID.  Results are defined bit for bit for finite costs and peak depths that are never exactly 0 (the MRF
 * branch's precondition); with these in force no negative zero can arise, so the order in which a minimum is reduced does
 * not affect the bits. */
typedef struct srh_mvs_sgm_params {
	double  beta, lambda;         /* 1, 1: the MRF branch's */
	double  phi_u, psi_u;         /* 0.5, 0.002 */
	int32_t path_mask;            /* 0xFF */
} srh_mvs_sgm_params;
void srh_mvs_sgm_params_defaults(srh_mvs_sgm_params *m);   /* needs no device */
/* The aggregation on the peaks srh_mvs_initial_estimate filled for this view (DEVICE buffer, w*h*top_k (cost, depth)
 * pairs; read only): writes the slot's depth map.  The counterpart of srh_mvs_mrf_estimate, with its argument checks.  A run
 * needs three blocks of w*h*16 doubles (peak depths, data costs, sums) + the labels in a scratch of its own (a later MRF run
 * leaves the state below alone and vice versa); when that does not fit the free device memory (option "mem_limit_mb"
 * honoured) the call fails with SRH_E_DEVICE and a message that names the bytes needed, before anything is queued, and the
 * depth map stays untouched.  The cancel flag is polled between directions; the depth map is written only by the read-off
 * after the last one.  info (paths, energy) may be NULL. */
int  srh_mvs_sgm_estimate(srh_context *ctx, int view_slot, int top_k, const void *peaks_dev,
                          const srh_mvs_sgm_params *m, srh_sgm_info *info);
/* srh_mvs_initial_estimate with the peaks kept in the context's own scratch, then srh_mvs_sgm_estimate on them. */
int  srh_mvs_initial_estimate_sgm(srh_context *ctx, int view_slot, const int32_t *neigh_slots, int nneigh,
                                  const srh_params *p, const srh_mvs_sgm_params *m, srh_sgm_info *info);
/* The same for several views at once, on the peaks kept by srh_mvs_initial_estimate_peaks: the views run side by side on the
 * per-view streams of srh_mvs_mrf_estimate_views, each with scratch of its own (one direction of one view does not fill the
 * chip), and each gets the bits of its single-view run.  infos: nviews entries, may be NULL. */
int  srh_mvs_sgm_estimate_views(srh_context *ctx, const int32_t *view_slots, int nviews, const srh_mvs_sgm_params *m, srh_sgm_info *infos);
/* State of the last srh_mvs_sgm_estimate on this context (the semantics and refusals of srh_mvs_mrf_state), to HOST buffers
 * (each may be NULL): labels (w*h), data_costs (w*h*(top_k+1): D), sums (w*h*(top_k+1): S).  There is no such state after
 * srh_mvs_sgm_estimate_views or after the view was uploaded again. */
int  srh_mvs_sgm_dims(srh_context *ctx, int *w, int *h, int *top_k);
int  srh_mvs_sgm_state(srh_context *ctx, int w, int h, int top_k, int32_t *labels, double *data_costs, double *sums);

/* ---- depth map -> point cloud ----
 * The output side of the path (the reference keeps only the PLY writer, multiviewstereo.cpp:291-315,
 * and the per-view coverage figure it logs, :402-421).  For every pixel of `slot` whose mask is WHITE and whose depth is
 * finite: the 3-D point unproject((x+0.5)/scale, (y+0.5)/scale) cut at that depth by pointFromDepth with the camera's
 * principal direction and centre -- the construction both cross-checks use (twoviewstereo.cpp:612-614,
 * multiviewstereo.cpp:688-692) -- and the pixel's colour.  HOST outputs, pixel order: xyz (w*h*3 doubles, NaN where
 * there is no point), rgb (w*h*3 bytes), valid (w*h bytes); each may be NULL.  *n_points = points produced,
 * *n_masked = pixels with a WHITE mask (coverage = finite depths / masked pixels is what the reference prints). */
int  srh_view_point_cloud(srh_context *ctx, int slot, const srh_params *p, double *xyz_out, uint8_t *rgb_out,
                          uint8_t *valid_out, int64_t *n_points, int64_t *n_masked, int64_t *n_finite);

/* ---- depth-map fusion: the views' depth maps -> one oriented cloud ----
 * NOT IN THE REFERENCE (it stops at outputPLYFile and hands its images to PMVS for a merged model); only the geometry is
 * the reference's: the point of a pixel is srh_view_point_cloud's, and the consistency test is that of
 * MultiViewStereo::crossCheck (multiviewstereo.cpp:666-729) applied to EVERY other view, the other view's mask consulted.
 *   points   pixel i of list entry v has a point P(v, i) when srh_view_point_cloud gives it one (mask WHITE, depth finite,
 *            pointFromDepth succeeds; the depth -1 has none).
 *   fusion   list entries in order v = 0 .. nviews-1, each strictly after the one before it.  For every pixel i of v with a point
 *            P1 that no earlier entry has claimed: the MEMBERS are (v, i) and, for every u != v in ascending u, the pixel
 *            j = (int)(y2)*w_u + (int)(x2) of (x2, y2) = image_scale * project_u(P1) when it lies inside u, has a point P2 and
 *            |P1 - P2| is finite and < thr (dist_threshold, or p->cross_check_threshold when that is <= 0); a claimed pixel
 *            still counts.  Fewer than min_views members: the pixel is UNSUPPORTED (nothing emitted, nothing claimed).
 *            Otherwise ONE point is emitted: the members' points added up in ascending list index (the first one starts the
 *            sum) / (double)m; per colour channel (2*sum + m)/(2*m) of the members' bytes in integers; nviews = m; and every
 *            member of an entry u > v is CLAIMED (it is not emitted when u's turn comes).
 *   normal   from v's own points: horizontal tangent P_R - P_L (both neighbours usable), else P_R - P, else P - P_L; the
 *            vertical one alike with P_D - P_U; a neighbour is usable inside the image, with a point and a depth within
 *            `gap` of the pixel's (normal_depth_gap, or 2*(max_depth - min_depth)/(num_depth_levels - 1) when that is <= 0).
 *            Both tangents and a finite cross product of length > 0: its unit vector, turned towards the camera centre
 *            (flags bit 0 set); else the unit vector from P to the camera centre (bit 0 clear).
 *   output   compacted in ascending (v, i) by an ordered stream compaction (no atomic decides a position): xyz, normal
 *            (3 doubles each), rgb (3 bytes), nviews, flags (1 byte each), src (2 int32: list index, pixel index).
 * The result is a pure function of the inputs: the same call gives the same bytes.  It stays in the context until the next
 * srh_mvs_fuse or srh_destroy (a later view upload does not touch it; a failed or cancelled srh_mvs_fuse leaves none).  The
 * call reads depth maps, masks, pixels and cameras and modifies none of them.  Views may differ in size; nviews == 1 with
 * min_views == 1 gives the view's own cloud.  All views must be in this one context (a sharded run: after
 * srh_comm_allgather_views they are).  The cancel hook is polled between the views. */
typedef struct srh_fuse_params {
	double  dist_threshold;     /* 0: p->cross_check_threshold */
	double  normal_depth_gap;   /* 0: two depth steps of p */
	int32_t min_views;          /* 2 */
	int32_t flags;              /* 0; reserved */
} srh_fuse_params;
void srh_fuse_params_defaults(srh_fuse_params *f);   /* 0, 0, 2, 0; needs no device */
/* n_candidates: pixels with a point, over all views = n_points + n_claimed + n_unsupported; n_normals: points with bit 0 */
typedef struct srh_fuse_info {
	int64_t n_points, n_candidates, n_claimed, n_unsupported, n_normals;
} srh_fuse_info;
/* f == NULL: the defaults; info may be NULL.  SRH_E_INVALID: nviews < 1, a duplicate or empty slot, min_views < 1. */
int  srh_mvs_fuse(srh_context *ctx, const int32_t *slots, int nviews, const srh_params *p, const srh_fuse_params *f,
                  srh_fuse_info *info);
int  srh_mvs_fused_count(srh_context *ctx, int64_t *n);
/* points [first, first + count) to HOST buffers, each may be NULL; a window outside [0, n]: SRH_E_INVALID */
int  srh_mvs_fused_download(srh_context *ctx, int64_t first, int64_t count, double *xyz, double *normals, uint8_t *rgb,
                            uint8_t *nviews, uint8_t *flags, int32_t *src);
/* the DEVICE arrays themselves (n entries each; null pointers when n == 0); each argument may be NULL */
int  srh_mvs_fused_device(srh_context *ctx, void **xyz, void **normals, void **rgb, void **nviews, void **flags, void **src);

/* ---- hole filling: TwoViewStereo::filterInvalidPixels (twoviewstereo.cpp:676-811) and weightedMedian (:821-860) ----
 * In place on `slot`'s depth map D, with the slot's image I and mask M; DESIGN.md 4b.
 *   SRH_FILTER_GAPS    the function's compiled body: per row, a run of isinf pixels with end - start < gap_width (the
 *                      reference's GAP_WIDTH_THRESHOLD is 2) is filled from both ends inward with the last non-inf value
 *                      before it and the first after it (NaN past the row's end), a non-finite one taking the other's
 *                      value.  NaN pixels are never gap-filled.  The result is G (without this flag G = D).
 *   SRH_FILTER_MEDIAN  its `#if 0` half: NaN where M is not WHITE; D where D (the map BEFORE the gap fill) is finite;
 *                      elsewhere weightedMedian of G over the support window of I at the pixel (p->weight_kind,
 *                      p->window_radius <= 5: else SRH_E_UNSUPPORTED): taps with a depth not NaN, inside
 *                      [min_depth, max_depth] and a weight > 1e-10, the libstdc++ heap's pop order, NaN for fewer than two.
 *                      The reference's loop also reads depths at taps OUTSIDE the image (another row, or past the map);
 *                      such a tap has the window weight exp(-geodesic_init/geodesic_sigma) (adaptive: 0) and the device
 *                      skips it, which is the reference's result only while that weight is not > 1e-10.  With
 *                      SRH_WEIGHT_GEODESIC and geodesic_sigma <= 0 or exp(-geodesic_init/geodesic_sigma) > 1e-10:
 *                      SRH_E_UNSUPPORTED, before anything is launched (srh_twoview_compute* under "filter_invalid" too).
 * Results are the same bits as the reference's loops.  Any slot works (MultiViewStereo views at radius 2 too); the
 * reference has this stage for TwoViewStereo (radius 5) only, the one parity target.  info may be NULL. */
enum { SRH_FILTER_GAPS = 1, SRH_FILTER_MEDIAN = 2 };
typedef struct srh_filter_info {
	int64_t holes;          /* WHITE pixels with a non-finite depth on entry */
	int64_t gap_filled;     /* pixels the gap fill wrote */
	int64_t median_filled;  /* holes the weighted median made finite */
	int64_t replayed;       /* holes whose median the exact replay of the heap selected (<= holes) */
} srh_filter_info;
int  srh_view_filter_invalid(srh_context *ctx, int slot, const srh_params *p, int flags, int gap_width,
                             srh_filter_info *info);

/* ---- speckle filter: small isolated regions of a depth map removed ----
 * NOT IN THE REFERENCE (other stereo stacks have it: OpenCV's filterSpeckles).  A connected-component size filter, in place
 * on `slot`'s depth map D (width w, height h) with the slot's mask M; it belongs between the cross-check and the hole
 * filling, which otherwise copies a small island of wrong depth into the holes around it.
 *   valid      a pixel with M == WHITE and isfinite(D) and D > 0.  The -1 of MultiViewStereo's "no peak" is therefore not
 *              valid and stays -1; +INF, -INF, NaN and masked pixels are never written.
 *   joined     two valid pixels that are 4-neighbours (left/right, up/down) are joined when fabs(Da - Db) <= max_diff,
 *              evaluated in double.  The test is symmetric, so the components are a pure function of the map.
 *   component  the transitive closure of the joins.  Its LABEL is the smallest linear pixel index y*w + x among its
 *              members, its SIZE its member count.
 *   removal    every pixel of a component with size < min_size is overwritten with the reject value: +INF (TwoViewStereo's
 *              value for a rejected pixel, which the gap fill and the median then treat as a hole), or NaN with the flag
 *              SRH_SPECKLE_TO_NAN (MultiViewStereo's cross-check value).  min_size <= 1 removes nothing.
 *   max_diff   <= 0: 2.0 * ((p->max_depth - p->min_depth) / (double)(p->num_depth_levels - 1)), the "two depth steps"
 *              srh_fuse_params.normal_depth_gap defaults to.
 * The result is a pure function of the inputs: the same call gives the same bytes, and a second call with the same
 * parameters removes nothing (removing a component neither joins nor splits the others).  labels_out (HOST, w*h int32, may
 * be NULL) receives per pixel the component label as computed BEFORE the removal, -1 for a pixel that is not valid.
 * s == NULL: the defaults; info may be NULL.  SRH_E_INVALID: an empty slot, min_size < 0, unknown flag bits, a max_diff
 * that is not finite, num_depth_levels < 2 when the default max_diff is asked for.  The call runs on the context's stream
 * and returns with the map updated; the cancel hook is polled between the launches (a cancelled call has not written D).
 * It reads the image of the slot not at all and leaves mask, image and the WTA by-products untouched. */
enum { SRH_SPECKLE_TO_NAN = 1 };
typedef struct srh_speckle_params {
	double  max_diff;           /* 0: two depth steps of p */
	int32_t min_size;           /* 0: off (nothing is removed) */
	int32_t flags;              /* 0, or SRH_SPECKLE_TO_NAN */
} srh_speckle_params;
void srh_speckle_params_defaults(srh_speckle_params *s);   /* 0, 0, 0; needs no device */
typedef struct srh_speckle_info {
	int64_t valid;               /* valid pixels on entry */
	int64_t components;          /* components on entry */
	int64_t removed_components;  /* components with size < min_size */
	int64_t removed_pixels;      /* their pixels: what the call overwrote */
	int64_t largest;             /* size of the largest component on entry (0: no valid pixel) */
} srh_speckle_info;
int  srh_view_filter_speckles(srh_context *ctx, int slot, const srh_params *p, const srh_speckle_params *s,
                              srh_speckle_info *info, int32_t *labels_out);

/* ---- rectification: a verged, distorted pair onto the row-aligned dense plan ----
 * NOT IN THE REFERENCE (a stereo library is expected to rectify: OpenCV's stereoRectify + remap).  The dense plan, the fast
 * path of srh_twoview_wta, is proposed only for two undistorted, non-refractive cameras with the same R, the same second and
 * third rows of K and a baseline along the camera x axis: srh_twoview_row_aligned is that very test (1 / 0; *fx_bx, may be
 * NULL, receives |fx * baseline| when 1).  Opt-in: nothing rectifies unless these entry points are called.
 *
 * srh_rectify_cameras (host math, needs no device): the rectified cameras ra, rb of the pair a, b, whose images (ALREADY
 * scaled by image_scale, as everywhere) are w x h pixels.  In this order of operations, C_v the centres, rows of R_v:
 *   r1 = (C_b - C_a)/|C_b - C_a|, negated if dot(r1, R_a.row0 + R_b.row0) < 0;   k = R_a.row2 + R_b.row2;
 *   r2 = cross(k, r1) normalised;   r3 = cross(r1, r2);   Rn = rows r1, r2, r3 -- the very same doubles for both cameras;
 *   Kn_v = [[f, 0, cx_v], [0, f, cy], [0, 0, 1]];   rv = srh_camera_from_krt(Kn_v, Rn, -Rn*C_v): no distortion, not refractive.
 *   focal 0 (auto):  the mean of K_a[0], K_a[4], K_b[0], K_b[4].
 *   cx_v NaN (auto): with d_v = Rn * R_v.row2 (the old optical axis in the new axes), (out_w/scale)/2 - f*d_v.x/d_v.z: the
 *                    old optical axis lands on the middle column.  PER VIEW by default: the rig test compares rows 2 and 3
 *                    of K only, and on a verged pair one shared cx pushes the object out of one frame.
 *                    SRH_RECTIFY_SHARED_CX replaces both auto values by their mean (the classic disparity geometry).
 *   cy NaN (auto):   (out_h/scale)/2 - f*mean_v(d_v.y/d_v.z).
 *   out_w, out_h 0:  w, h.  They are the size of the rectified views in scaled pixels; only the auto principal point reads them here.
 * SRH_E_INVALID: null pointers, w or h <= 0, image_scale <= 0, a negative or oversized output size, unknown flag bits, a
 * focal or principal point that is not finite, coincident centres.  SRH_E_UNSUPPORTED: a refractive camera (no homography
 * rectifies it); |cross(k, r1)| < 1e-6*|k| (the baseline runs along the viewing direction: forward motion); d_v.z <= 0.1 for
 * either view (it looks more than 84 degrees away from the rectified axis).
 *
 * srh_view_rectify_map: where destination pixel (x, y) of a rectified view of out_w x out_h pixels with camera rect_cam reads
 * the image of src_slot: uv_out (HOST, out_w*out_h pairs) receives (u, v) in the source's scaled raster, pixel centres at
 * integers.  With s = image_scale:  ray = unproject(rect_cam, (x+0.5)/s, (y+0.5)/s);  P = ray.src + ray.dir;
 * q = project(src camera, P);  u = q.x*s - 0.5, v = q.y*s - 0.5, where a value within 1e-11*(1 + |value|) of an integer is
 * that integer (the round trip leaves about 1e-14 of noise: a whole-pixel shift then comes through byte for byte);  (NaN,
 * NaN) where P lies behind the source camera or u, v are not finite.  The source camera may be distorted; a refractive one is SRH_E_UNSUPPORTED.
 *
 * srh_twoview_rectify: the views of src_a, src_b warped into dst_a, dst_b with the cameras of srh_rectify_cameras (r NULL:
 * the defaults; p supplies image_scale).  Per destination pixel with a finite (u, v):  x0 = floor(u), y0 = floor(v) (saturating),
 * a = u - x0, b = v - y0;  every one of the four channels is
 *   floor(((1-a)*c00 + a*c10)*(1-b) + ((1-a)*c01 + a*c11)*b + 0.5) clamped to [0, 255], in double, no fused multiply-add,
 * from the four taps CLAMPED into the source; the pixel is WHITE iff the four taps lie inside the source unclamped and are
 * WHITE there -- where a tap whose weight is exactly 0 (a == 0: the right column, b == 0: the lower row) is not asked, so
 * that a whole-pixel shift keeps its last column and row.  Elsewhere bytes 0,0,0,0 and not WHITE.  A destination slot then is what srh_view_upload of those pixels,
 * that mask and the rectified camera leaves: derived planes recomputed, depth NaN, WTA by-products and peaks forgotten.
 * Both warps are queued before either slot is written, so dst == src is legal (the four slots otherwise distinct per
 * role: src_a != src_b, dst_a != dst_b).  A refusal leaves all four slots as they were.  info (may be NULL): the angle
 * (radians) between each view's old optical axis and the rectified one, the WHITE pixels of each result, and fx_bx of the
 * rectified pair.
 *
 * srh_view_depth_unrectify: the depth map of rect_slot (a rectified view; z along the rectified axis) brought into
 * dst_slot (the view the user handed in: same centre within 1e-9*(1+|C|), else SRH_E_INVALID; may be distorted), written
 * into dst_slot's depth map.  Per WHITE pixel (x, y) of dst:  ray = unproject(dst camera, (x+0.5)/s, (y+0.5)/s);
 * q = project(rectified camera, ray.src + ray.dir);  (x2, y2) = (q.x*s, q.y*s);  behind the rectified camera or outside
 * [0, w_r) x [0, h_r): depth NaN, index -1;  else dr = depth_rect[trunc(y2)][trunc(x2)] (the cross-check's pixel rule), copied
 * through unchanged when it is not finite or <= 0 (+INF, NaN, MultiViewStereo's -1), else X = ray.src + ray.dir*(dr / dot(r3,
 * ray.dir)) and the depth is dst's local z of X.  Pixels that are not WHITE get NaN.  src_index_out (HOST, w*h int32 of dst,
 * may be NULL): trunc(y2)*w_r + trunc(x2), or -1.  Nearest-pixel on purpose: depth maps carry +INF / NaN classes that no
 * interpolation keeps. */
enum { SRH_RECTIFY_SHARED_CX = 1 };
typedef struct srh_rectify_params {
	double  focal;              /* 0: auto */
	double  cx_a, cx_b, cy;     /* NaN: auto */
	int32_t out_w, out_h;       /* 0: the size of view a; scaled pixels */
	int32_t flags, reserved;    /* 0, or SRH_RECTIFY_SHARED_CX */
} srh_rectify_params;
void srh_rectify_params_defaults(srh_rectify_params *r);   /* 0, NaN, NaN, NaN, 0, 0, 0, 0; NULL ignored; needs no device */
int  srh_rectify_cameras(const srh_camera *a, const srh_camera *b, int w, int h, double image_scale,
                         const srh_rectify_params *r, srh_camera *ra, srh_camera *rb);
int  srh_twoview_row_aligned(const srh_camera *a, const srh_camera *b, double *fx_bx);
typedef struct srh_rectify_info {
	double  angle_a, angle_b;   /* radians between the old and the rectified optical axis */
	double  fx_bx;              /* of the rectified pair */
	int64_t white_a, white_b;   /* WHITE pixels of the rectified views */
} srh_rectify_info;
int  srh_twoview_rectify(srh_context *ctx, int src_a, int src_b, int dst_a, int dst_b, const srh_params *p,
                         const srh_rectify_params *r, srh_rectify_info *info);
int  srh_view_rectify_map(srh_context *ctx, int src_slot, const srh_camera *rect_cam, int out_w, int out_h,
                          double image_scale, double *uv_out);
int  srh_view_depth_unrectify(srh_context *ctx, int rect_slot, int dst_slot, const srh_params *p, int32_t *src_index_out);

/* ---- epipolar curves ----
 * TwoViewStereo::epipolarCurve (public member, twoviewstereo.hpp:66-70, twoviewstereo.cpp:999-1054;
 * the GUI's curve preview calls it, stereowidget.cpp:621-672) when mvs == 0, and
 * MultiViewStereo::epipolarCurve (multiviewstereo.cpp:754-810: uniform depths, clipped segments,
 * consecutive duplicates removed) when mvs != 0.  For each of the `nqueries` reference pixels
 * xy[2q], xy[2q+1] of slot `ref_slot`: the candidate pixels in slot `oth_slot`, in the order the
 * reference visits them, written as (x,y) int32 pairs to out_xy + q*2*max_pts; counts[q] receives
 * the curve length (which may exceed max_pts; only max_pts points are written).  The reference
 * pixel's own mask is not consulted (the callers do that).  All pointers are HOST memory. */
int  srh_epipolar_curves(srh_context *ctx, int ref_slot, int oth_slot, const srh_params *p, int mvs,
                         int nqueries, const int32_t *xy, int32_t *out_xy, int max_pts, int32_t *counts);

/* ---- GUI-side users of the camera model ----
 * StereoWidget::epipolarLineItem (gui/widgets/stereowidget.cpp:621-672): the curve preview drawn while the user moves
 * over the left image.  For each of the nqueries pixels xy[2q], xy[2q+1] (image coordinates as the GUI has them: no
 * +0.5, no scale): num_depths UNIFORM depths in [min_depth, max_depth], plane Plane3d(principal direction, depth),
 * projection into `oth_slot`; a point becomes a vertex of the path when it is more than one pixel from the last one.
 * out_xy: nqueries*num_depths*2 doubles (the vertices of query q start at q*num_depths*2), counts[q] = vertices
 * (0: nothing to draw).  HOST pointers. */
int  srh_epipolar_preview(srh_context *ctx, int ref_slot, int oth_slot, double min_depth, double max_depth, int num_depths,
                          int nqueries, const double *xy, double *out_xy, int32_t *counts);
/* RefractionCalibration::error / totalError (stereo/refractioncalibration.cpp:175-199, 408-469): for npairs
 * correspondences (p1 in slot1's image, p2 in slot2's): the ray-ray distance scaled to image space, per pair
 * (err_out, may be NULL: diff()'s single component -- RefractionCalibration::error is its absolute value), the sum
 * of its squares in pair order (*total) and total / npairs (*average, NaN for no pairs); the cameras are those
 * uploaded with the slots (re-upload a view to try other interface parameters: the LM loop above stays host code). */
int  srh_refraction_error(srh_context *ctx, int slot1, int slot2, int npairs, const double *p1_xy, const double *p2_xy,
                          double *err_out, double *total, double *average);

/* ---- multi-GPU exchange (RCCL over xGMI; one process and one context per GPU) ----
 * srh_comm_unique_id: rank 0 creates the 128-byte id and hands it to the other ranks by any
 * means (MPI, files, torch.distributed ...).  srh_comm_init is collective.  librccl is loaded on
 * first use; SRH_E_UNSUPPORTED if it is absent. */
#define SRH_COMM_ID_BYTES 128
int  srh_comm_unique_id(void *id_out);
/* The communicator is non-blocking (ncclConfig_t::blocking = 0): a rank that never arrives at the rendezvous, or a call
 * that stays "in progress" longer than the timeout (srh_comm_set_timeout_ms, default 120 000 ms), returns SRH_E_DEVICE
 * after the communicator has been aborted -- a missing rank ends the job with an error instead of hanging it. */
int  srh_comm_init(srh_context *ctx, int nranks, int rank, const void *id);
int  srh_comm_set_timeout_ms(int ms);
/* NCCL_VERSION_CODE of the loaded librccl (ncclGetVersion), 0 when there is none; what the context's communicator
 * spans (0 ranks, rank -1 without one) */
int  srh_comm_version(void);
int  srh_comm_info(srh_context *ctx, int *nranks, int *rank);
/* Gather the depth map of `slot` (w*h doubles, equal on all ranks) to `root`:
 * recv_dev (DEVICE, nranks*w*h doubles, rank order) is written on the root only. */
int  srh_comm_gather_depth(srh_context *ctx, int slot, int root, void *recv_dev);
/* Every rank receives every rank's map of `slot` (MVS cross-check input). */
int  srh_comm_allgather_depth(srh_context *ctx, int slot, void *recv_dev);
/* The same collective on HOST buffers: every rank contributes `count` doubles and receives nranks*count (rank
 * order); staged through device memory of the context, RCCL in between.  For callers above the C-ABI that hold
 * several maps per rank in host memory (host/sharded.hpp). */
int  srh_comm_allgather_host(srh_context *ctx, const double *send_host, size_t count, double *recv_host);
/* The one exchange of a sharded MultiViewStereo::runTask, device to device: the nviews views are dealt to the ranks in
 * contiguous balanced shards (view v belongs to the rank r with lo(r) <= v < hi(r), lo(r) = r*(n/world) + min(r, n%world));
 * every rank contributes the depth maps of ITS views, and on return (stream-ordered, nothing is staged through host
 * memory) the depth map of every slot on every rank is its owner's.  Views may differ in size (maps travel padded). */
int  srh_comm_allgather_views(srh_context *ctx, const int32_t *view_slots, int nviews);
int  srh_comm_destroy(srh_context *ctx);

/* ---- measurement ---- */
int  srh_get_stats(srh_context *ctx, srh_stats *out);
/* When enabled every kernel launch is bracketed by hipEvents on the context
 * stream; durations are accumulated per kernel name. */
int  srh_profile_enable(srh_context *ctx, int on);
int  srh_profile_reset(srh_context *ctx);
/* total_ms / launches of kernel `name`; returns SRH_E_INVALID if never launched. */
int  srh_profile_get(srh_context *ctx, const char *name, double *total_ms, int64_t *launches);
/* Writes up to cap bytes of "name total_ms launches\n" lines. */
int  srh_profile_dump(srh_context *ctx, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* STEREO_RECON_HIP_H */
