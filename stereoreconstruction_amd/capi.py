"""ctypes binding of include/stereo_recon_hip.h (libstereo_recon_hip.so).

This is the ONLY compute path of the package: there is no CPU / numpy fallback.
If the shared library is missing the import of :func:`lib` raises, and if no HIP
device is present :class:`Context` raises ``StereoHipError`` (SRH_E_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRH_LIBRARY names another build of the same library (the -DSRH_PROFILE_PHASES diagnostic build)
LIB_PATH = os.environ.get("SRH_LIBRARY") or os.path.join(_HERE, "libstereo_recon_hip.so")

SRH_OK = 0
SRH_E_INVALID, SRH_E_DEVICE, SRH_E_NO_DEVICE, SRH_E_CANCELLED, SRH_E_UNSUPPORTED = -1, -2, -3, -4, -5
WEIGHT_ADAPTIVE, WEIGHT_GEODESIC = 0, 1
MAX_VIEWS = 64
MAX_VIEW_DIM = 32767              # SRH_MAX_VIEW_DIM: the largest width / height upload accepts

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class Camera(C.Structure):
    """srh_camera"""
    _fields_ = [
        ("K", C.c_double * 9), ("Kinv", C.c_double * 9), ("R", C.c_double * 9), ("Rinv", C.c_double * 9),
        ("t", C.c_double * 3), ("C", C.c_double * 3),
        ("dist", C.c_double * 5),
        ("is_distorted", C.c_int32), ("is_refractive", C.c_int32),
        ("plane_normal", C.c_double * 3), ("plane_dist", C.c_double), ("refr_index", C.c_double),
        ("pdir", C.c_double * 3),
    ]


class Params(C.Structure):
    """srh_params"""
    _fields_ = [
        ("min_depth", C.c_double), ("max_depth", C.c_double),
        ("num_depth_levels", C.c_int32), ("window_radius", C.c_int32),
        ("image_scale", C.c_double),
        ("weight_kind", C.c_int32), ("geodesic_iters", C.c_int32),
        ("geodesic_sigma", C.c_double), ("geodesic_init", C.c_double),
        ("adaptive_color_sigma", C.c_double), ("weight_cutoff", C.c_double),
        ("bad_ret", C.c_double), ("max_color_diff", C.c_double),
        ("second_best_factor", C.c_double), ("wta_margin", C.c_double),
        ("inconsistency_thresh", C.c_double),
        ("peak_threshold", C.c_double), ("cross_check_threshold", C.c_double),
        ("neighbour_min_dot", C.c_double),
        ("top_k", C.c_int32), ("num_neighbours", C.c_int32),
    ]


class SrhMrfParams(C.Structure):
    _fields_ = [("beta", C.c_double), ("lambda_", C.c_double), ("phi_u", C.c_double), ("psi_u", C.c_double),
                ("max_iters", C.c_int32), ("min_energy_drop", C.c_double)]


class SrhMrfInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("energy_initial", C.c_double), ("energy_final", C.c_double)]


class SrhTwoviewMrfParams(C.Structure):
    """srh_twoview_mrf_params"""
    _fields_ = [("smooth_exp", C.c_int32), ("smooth_max", C.c_double), ("lambda_", C.c_double),
                ("max_iters", C.c_int32), ("min_energy_drop", C.c_double)]


class SrhTwoviewSgmParams(C.Structure):
    """srh_twoview_sgm_params"""
    _fields_ = [("smooth_exp", C.c_int32), ("smooth_max", C.c_double), ("lambda_", C.c_double), ("path_mask", C.c_int32)]


class SrhSgmInfo(C.Structure):
    """srh_sgm_info"""
    _fields_ = [("paths", C.c_int32), ("energy", C.c_double)]


class SrhMvsSgmParams(C.Structure):
    """srh_mvs_sgm_params"""
    _fields_ = [("beta", C.c_double), ("lambda_", C.c_double), ("phi_u", C.c_double), ("psi_u", C.c_double),
                ("path_mask", C.c_int32)]


# what srh_twoview_label_costs writes for a label without a pixel (SRH_LABEL_PIXEL_NONE)
LABEL_PIXEL_NONE = -2147483648

# option "arith" (include/stereo_recon_hip.h)
ARITH_EXACT, ARITH_FMA, ARITH_F32, ARITH_CERTIFIED = 0, 1, 2, 3
ARITH_DEFAULT = ARITH_CERTIFIED


class Stats(C.Structure):
    """srh_stats"""
    _fields_ = [("n_pixels", C.c_int64), ("n_eval", C.c_int64), ("n_eval_device", C.c_int64),
                ("used_dense_path", C.c_int32), ("used_fused_kernel", C.c_int32),
                ("used_strip_kernel", C.c_int32), ("band_retries", C.c_int32),
                ("n_certified", C.c_int64), ("n_flagged", C.c_int64), ("band_budget_bytes", C.c_int64),
                ("mvs_waves_staged", C.c_int64), ("mvs_waves_listed", C.c_int64),
                ("scan_tiles_template", C.c_int64), ("scan_tiles_walked", C.c_int64),
                ("scan_tiles_bound", C.c_int64)]


class FilterInfo(C.Structure):
    """srh_filter_info"""
    _fields_ = [("holes", C.c_int64), ("gap_filled", C.c_int64), ("median_filled", C.c_int64), ("replayed", C.c_int64)]


# srh_view_filter_invalid flags
FILTER_GAPS, FILTER_MEDIAN = 1, 2


class FuseParams(C.Structure):
    """srh_fuse_params"""
    _fields_ = [("dist_threshold", C.c_double), ("normal_depth_gap", C.c_double), ("min_views", C.c_int32), ("flags", C.c_int32)]


class FuseInfo(C.Structure):
    """srh_fuse_info"""
    _fields_ = [("n_points", C.c_int64), ("n_candidates", C.c_int64), ("n_claimed", C.c_int64),
                ("n_unsupported", C.c_int64), ("n_normals", C.c_int64)]


class SpeckleParams(C.Structure):
    """srh_speckle_params"""
    _fields_ = [("max_diff", C.c_double), ("min_size", C.c_int32), ("flags", C.c_int32)]


class SpeckleInfo(C.Structure):
    """srh_speckle_info"""
    _fields_ = [("valid", C.c_int64), ("components", C.c_int64), ("removed_components", C.c_int64),
                ("removed_pixels", C.c_int64), ("largest", C.c_int64)]


class SubpixelInfo(C.Structure):
    """srh_subpixel_info"""
    _fields_ = [("n_class", C.c_int64 * 5), ("n_moved", C.c_int64)]


class MvsSubpixelInfo(C.Structure):
    """srh_mvs_subpixel_info"""
    _fields_ = [("n_class", C.c_int64 * 6), ("n_moved", C.c_int64), ("n_fallback", C.c_int64)]


# srh_view_filter_speckles flag: the reject value is NaN, not +INF
SPECKLE_TO_NAN = 1


class RectifyParams(C.Structure):
    """srh_rectify_params"""
    _fields_ = [("focal", C.c_double), ("cx_a", C.c_double), ("cx_b", C.c_double), ("cy", C.c_double),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class RectifyInfo(C.Structure):
    """srh_rectify_info"""
    _fields_ = [("angle_a", C.c_double), ("angle_b", C.c_double), ("fx_bx", C.c_double),
                ("white_a", C.c_int64), ("white_b", C.c_int64)]


# srh_rectify_params flag: one principal-point column for both rectified views (the mean of the two auto values)
RECTIFY_SHARED_CX = 1

# srh_mvs_fuse: bit 0 of a fused point's flags
FUSE_HAS_NORMAL = 1

# option "cost" / srh_twoview_pair_costs kind: TwoViewStereo::cost_ncc, cost_sad; the support-weighted census cost (not in
# the reference; 2 is no cost)
COST_NCC, COST_SAD = 0, 1
COST_CENSUS = 3

# option "wta_outputs": the by-products of the WTA scan a pass keeps (SRH_WTA_*)
WTA_WINNERS, WTA_COSTS = 1, 2
# option "subpixel": what the refinement did to a pixel (SRH_SUBPX_*)
SUBPX_NONE, SUBPX_NO_NEIGHBOUR, SUBPX_FLAT, SUBPX_OUTSIDE, SUBPX_REFINED = 0, 1, 2, 3, 4
# srh_mvs_view_subpixel only: the depth is no candidate depth of the neighbours given
SUBPX_NO_WINNER = 5
# scaling at file resolution (SRH_SCALE_*, SRH_MASK_*)
SCALE_SMOOTH, SCALE_FAST = 0, 1
MASK_NONE, MASK_ALPHA_FAST, MASK_IMAGE_SMOOTH = 0, 1, 2


PROGRESS_FN = C.CFUNCTYPE(None, C.c_int, C.c_char_p, C.c_void_p)

# every symbol include/stereo_recon_hip.h declares
EXPORTS = [
    "srh_abi_version", "srh_build_id", "srh_last_error", "srh_device_count", "srh_hw_queues_requested",
    "srh_params_twoview_defaults", "srh_params_mvs_defaults", "srh_camera_from_krt", "srh_camera_from_p",
    "srh_mvs_neighbours", "srh_cert_bound", "srh_cert_sigma3", "srh_tscan_bound",
    "srh_create", "srh_destroy", "srh_set_stream", "srh_set_hooks", "srh_synchronize", "srh_set_option",
    "srh_view_upload", "srh_view_size", "srh_scaled_size", "srh_image_scale", "srh_view_upload_scaled", "srh_view_image_download",
    "srh_view_depth_download", "srh_view_depth_upload", "srh_view_census",
    "srh_view_depth_device_ptr", "srh_view_depth_copy_to_device", "srh_view_depth_copy_from_device",
    "srh_view_wta_outputs", "srh_view_wta_outputs_device", "srh_view_wta_outputs_state",
    "srh_view_subpixel", "srh_view_subpixel_device", "srh_view_subpixel_info", "srh_mvs_view_subpixel",
    "srh_twoview_wta", "srh_twoview_cross_check", "srh_twoview_compute", "srh_twoview_cost_rows", "srh_twoview_pair_costs", "srh_debug_exp",
    "srh_mvs_initial_estimate", "srh_mvs_cross_check", "srh_view_point_cloud", "srh_view_filter_invalid",
    "srh_speckle_params_defaults", "srh_view_filter_speckles",
    "srh_rectify_params_defaults", "srh_rectify_cameras", "srh_twoview_row_aligned", "srh_twoview_rectify",
    "srh_view_rectify_map", "srh_view_depth_unrectify",
    "srh_fuse_params_defaults", "srh_mvs_fuse", "srh_mvs_fused_count", "srh_mvs_fused_download", "srh_mvs_fused_device",
    "srh_epipolar_curves",
    "srh_epipolar_preview", "srh_refraction_error",
    "srh_mrf_params_defaults", "srh_mvs_mrf_estimate", "srh_mvs_mrf_state", "srh_mvs_mrf_dims", "srh_mvs_initial_estimate_mrf",
    "srh_mvs_initial_estimate_peaks", "srh_mvs_mrf_estimate_views",
    "srh_twoview_mrf_params_defaults", "srh_twoview_label_costs", "srh_twoview_mrf_optimize", "srh_twoview_mrf",
    "srh_twoview_compute_mrf", "srh_twoview_mrf_dims", "srh_twoview_mrf_state",
    "srh_twoview_sgm_params_defaults", "srh_twoview_sgm_aggregate", "srh_twoview_sgm", "srh_twoview_compute_sgm",
    "srh_twoview_sgm_dims", "srh_twoview_sgm_state",
    "srh_mvs_sgm_params_defaults", "srh_mvs_sgm_estimate", "srh_mvs_initial_estimate_sgm", "srh_mvs_sgm_estimate_views",
    "srh_mvs_sgm_dims", "srh_mvs_sgm_state",
    "srh_comm_unique_id", "srh_comm_init", "srh_comm_gather_depth", "srh_comm_allgather_depth", "srh_comm_allgather_host",
    "srh_comm_allgather_views",
    "srh_comm_destroy", "srh_comm_set_timeout_ms", "srh_comm_version", "srh_comm_info",
    "srh_get_stats", "srh_profile_enable", "srh_profile_reset", "srh_profile_get", "srh_profile_dump",
]


class CertInfo(C.Structure):
    _fields_ = [("e0", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("k3", C.c_double), ("zmax2", C.c_double),
                ("m_hi", C.c_double), ("ok", C.c_int32), ("taps", C.c_int32)]


class TscanBoundInfo(C.Structure):
    """srh_tscan_bound_info"""
    _fields_ = [("E", C.c_double), ("eU", C.c_double), ("eU_template", C.c_double), ("dyU", C.c_double),
                ("room_col", C.c_double), ("room_one", C.c_double), ("room_proj", C.c_double),
                ("pixel_ok", C.c_int32), ("template_ok", C.c_int32), ("passes", C.c_int32), ("pad_", C.c_int32)]


class StereoHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("srh error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load libstereo_recon_hip.so; raises OSError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not found: build it with `make -C stereoreconstruction_amd/csrc` "
                      "(or __graft_entry__.build()); there is no fallback path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.srh_abi_version.restype = C.c_int
    L.srh_build_id.restype = C.c_char_p
    L.srh_last_error.restype = C.c_char_p
    L.srh_device_count.argtypes = [C.POINTER(C.c_int)]
    L.srh_params_twoview_defaults.argtypes = [C.POINTER(Params)]
    L.srh_params_twoview_defaults.restype = None
    L.srh_params_mvs_defaults.argtypes = [C.POINTER(Params)]
    L.srh_params_mvs_defaults.restype = None
    L.srh_camera_from_krt.argtypes = [c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                      C.c_double, C.c_double, C.POINTER(Camera)]
    L.srh_camera_from_p.argtypes = [c_double_p, c_double_p, c_double_p, C.c_double, C.c_double, C.POINTER(Camera)]
    L.srh_mvs_neighbours.argtypes = [C.c_int, C.POINTER(Camera), C.POINTER(Params), c_int32_p, c_int32_p]
    L.srh_cert_bound.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(CertInfo)]
    L.srh_cert_sigma3.argtypes = [C.POINTER(Params), C.c_int, C.c_double]
    L.srh_cert_sigma3.restype = C.c_double
    L.srh_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.srh_destroy.argtypes = [vp]
    L.srh_destroy.restype = None
    L.srh_set_stream.argtypes = [vp, vp]
    L.srh_set_hooks.argtypes = [vp, C.POINTER(C.c_int), PROGRESS_FN, vp]
    L.srh_synchronize.argtypes = [vp]
    L.srh_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.srh_view_upload.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_uint8_p, c_uint8_p, C.POINTER(Camera)]
    L.srh_view_size.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_scaled_size.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_image_scale.argtypes = [vp, c_uint8_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, c_uint8_p,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_view_upload_scaled.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_uint8_p, C.c_int, c_uint8_p, C.c_int, C.c_int, C.c_int,
                                         C.c_double, C.c_int, C.POINTER(Camera)]
    L.srh_view_image_download.argtypes = [vp, C.c_int, c_uint8_p, c_uint8_p]
    L.srh_view_depth_download.argtypes = [vp, C.c_int, c_double_p]
    L.srh_view_depth_upload.argtypes = [vp, C.c_int, c_double_p]
    L.srh_view_census.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64)]
    L.srh_view_depth_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.srh_view_wta_outputs.argtypes = [vp, C.c_int, c_int32_p, c_int32_p, c_double_p, c_double_p]
    L.srh_view_wta_outputs_device.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.srh_view_wta_outputs_state.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_view_subpixel.argtypes = [vp, C.c_int, c_double_p, c_int32_p, C.POINTER(C.c_uint8)]
    L.srh_view_subpixel_device.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.srh_view_subpixel_info.argtypes = [vp, C.c_int, C.POINTER(SubpixelInfo)]
    L.srh_mvs_view_subpixel.argtypes = [vp, C.c_int, c_int32_p, C.c_int, C.POINTER(Params), C.POINTER(MvsSubpixelInfo),
                                        c_double_p, c_int32_p, c_int32_p, C.POINTER(C.c_uint8)]
    L.srh_mrf_params_defaults.argtypes = [C.POINTER(SrhMrfParams)]
    L.srh_mrf_params_defaults.restype = None
    L.srh_mvs_mrf_estimate.argtypes = [vp, C.c_int, C.c_int, C.c_void_p, C.POINTER(SrhMrfParams), C.POINTER(SrhMrfInfo)]
    L.srh_mvs_initial_estimate_mrf.argtypes = [vp, C.c_int, c_int32_p, C.c_int, C.POINTER(Params), C.POINTER(SrhMrfParams), C.POINTER(SrhMrfInfo)]
    L.srh_mvs_initial_estimate_peaks.argtypes = [vp, C.c_int, c_int32_p, C.c_int, C.POINTER(Params)]
    L.srh_mvs_mrf_estimate_views.argtypes = [vp, c_int32_p, C.c_int, C.POINTER(SrhMrfParams), C.POINTER(SrhMrfInfo)]
    L.srh_mvs_mrf_state.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_double_p, c_double_p]
    L.srh_mvs_mrf_dims.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    tmp = C.POINTER(SrhTwoviewMrfParams)
    L.srh_twoview_mrf_params_defaults.argtypes = [tmp]
    L.srh_twoview_mrf_params_defaults.restype = None
    L.srh_twoview_label_costs.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int, c_double_p, c_int32_p]
    L.srh_twoview_mrf_optimize.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_int, C.c_void_p, tmp, C.POINTER(SrhMrfInfo)]
    L.srh_twoview_mrf.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), tmp, C.POINTER(SrhMrfInfo)]
    L.srh_twoview_compute_mrf.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), tmp, c_double_p, c_double_p, C.POINTER(SrhMrfInfo)]
    L.srh_twoview_mrf_dims.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_twoview_mrf_state.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_double_p, c_double_p]
    tsp = C.POINTER(SrhTwoviewSgmParams)
    L.srh_twoview_sgm_params_defaults.argtypes = [tsp]
    L.srh_twoview_sgm_params_defaults.restype = None
    L.srh_twoview_sgm_aggregate.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_int, C.c_void_p, tsp, C.POINTER(SrhSgmInfo)]
    L.srh_twoview_sgm.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), tsp, C.POINTER(SrhSgmInfo)]
    L.srh_twoview_compute_sgm.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), tsp, c_double_p, c_double_p, C.POINTER(SrhSgmInfo)]
    L.srh_twoview_sgm_dims.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_twoview_sgm_state.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_double_p, c_double_p]
    msp = C.POINTER(SrhMvsSgmParams)
    L.srh_mvs_sgm_params_defaults.argtypes = [msp]
    L.srh_mvs_sgm_params_defaults.restype = None
    L.srh_mvs_sgm_estimate.argtypes = [vp, C.c_int, C.c_int, C.c_void_p, msp, C.POINTER(SrhSgmInfo)]
    L.srh_mvs_initial_estimate_sgm.argtypes = [vp, C.c_int, c_int32_p, C.c_int, C.POINTER(Params), msp, C.POINTER(SrhSgmInfo)]
    L.srh_mvs_sgm_estimate_views.argtypes = [vp, c_int32_p, C.c_int, msp, C.POINTER(SrhSgmInfo)]
    L.srh_mvs_sgm_dims.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_mvs_sgm_state.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_double_p, c_double_p]
    L.srh_comm_allgather_views.argtypes = [vp, c_int32_p, C.c_int]
    L.srh_hw_queues_requested.restype = C.c_int
    L.srh_epipolar_preview.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, c_double_p, c_double_p, c_int32_p]
    L.srh_refraction_error.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.srh_view_point_cloud.argtypes = [vp, C.c_int, C.POINTER(Params), c_double_p, c_uint8_p, c_uint8_p, vp, vp, vp]
    L.srh_view_filter_invalid.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_int, C.c_int, C.POINTER(FilterInfo)]
    L.srh_speckle_params_defaults.argtypes = [C.POINTER(SpeckleParams)]
    L.srh_speckle_params_defaults.restype = None
    L.srh_view_filter_speckles.argtypes = [vp, C.c_int, C.POINTER(Params), C.POINTER(SpeckleParams), C.POINTER(SpeckleInfo), c_int32_p]
    L.srh_rectify_params_defaults.argtypes = [C.POINTER(RectifyParams)]
    L.srh_rectify_params_defaults.restype = None
    L.srh_rectify_cameras.argtypes = [C.POINTER(Camera), C.POINTER(Camera), C.c_int, C.c_int, C.c_double, C.POINTER(RectifyParams),
                                      C.POINTER(Camera), C.POINTER(Camera)]
    L.srh_twoview_row_aligned.argtypes = [C.POINTER(Camera), C.POINTER(Camera), c_double_p]
    L.srh_twoview_rectify.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(RectifyParams),
                                      C.POINTER(RectifyInfo)]
    L.srh_view_rectify_map.argtypes = [vp, C.c_int, C.POINTER(Camera), C.c_int, C.c_int, C.c_double, c_double_p]
    L.srh_view_depth_unrectify.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), c_int32_p]
    L.srh_fuse_params_defaults.argtypes = [C.POINTER(FuseParams)]
    L.srh_fuse_params_defaults.restype = None
    L.srh_mvs_fuse.argtypes = [vp, c_int32_p, C.c_int, C.POINTER(Params), C.POINTER(FuseParams), C.POINTER(FuseInfo)]
    L.srh_mvs_fused_count.argtypes = [vp, C.POINTER(C.c_int64)]
    L.srh_mvs_fused_download.argtypes = [vp, C.c_int64, C.c_int64, c_double_p, c_double_p, c_uint8_p, c_uint8_p, c_uint8_p, c_int32_p]
    L.srh_mvs_fused_device.argtypes = [vp] + [C.POINTER(vp)] * 6
    L.srh_twoview_pair_costs.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int, c_int32_p, c_double_p]
    L.srh_view_depth_copy_to_device.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.srh_view_depth_copy_from_device.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.srh_twoview_wta.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int]
    L.srh_twoview_cross_check.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params)]
    L.srh_twoview_cost_rows.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, c_double_p, C.c_size_t,
                                        c_int32_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_twoview_compute.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), c_double_p, c_double_p]
    L.srh_debug_exp.argtypes = [vp, c_double_p, C.c_int, c_double_p, c_double_p]
    L.srh_mvs_initial_estimate.argtypes = [vp, C.c_int, c_int32_p, C.c_int, C.POINTER(Params), C.c_int, C.c_int, vp]
    L.srh_mvs_cross_check.argtypes = [vp, c_int32_p, C.c_int, C.c_int, C.POINTER(Params)]
    L.srh_epipolar_curves.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int, c_int32_p,
                                      c_int32_p, C.c_int, c_int32_p]
    L.srh_comm_unique_id.argtypes = [vp]
    L.srh_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.srh_comm_gather_depth.argtypes = [vp, C.c_int, C.c_int, vp]
    L.srh_comm_allgather_depth.argtypes = [vp, C.c_int, vp]
    L.srh_comm_allgather_host.argtypes = [vp, c_double_p, C.c_size_t, c_double_p]
    L.srh_comm_destroy.argtypes = [vp]
    L.srh_comm_set_timeout_ms.argtypes = [C.c_int]
    L.srh_comm_version.restype = C.c_int
    L.srh_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.srh_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.srh_profile_enable.argtypes = [vp, C.c_int]
    L.srh_profile_reset.argtypes = [vp]
    L.srh_profile_get.argtypes = [vp, C.c_char_p, c_double_p, C.POINTER(C.c_int64)]
    L.srh_profile_dump.argtypes = [vp, C.c_char_p, C.c_size_t]
    _lib = L
    return L


def _check(rc):
    if rc != SRH_OK:
        raise StereoHipError(rc, lib().srh_last_error().decode("utf-8", "replace"))


def _dptr(a):
    return a.ctypes.data_as(c_double_p)


def params_twoview(**kw):
    p = Params()
    lib().srh_params_twoview_defaults(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def mrf_params(**kw):
    """srh_mrf_params with the reference's constants (multiviewstereo.cpp:98-101, 631, 641)."""
    m = SrhMrfParams()
    lib().srh_mrf_params_defaults(C.byref(m))
    for k, v in kw.items():
        setattr(m, "lambda_" if k == "lambda" else k, v)
    return m


def twoview_mrf_params(**kw):
    """srh_twoview_mrf_params with the reference's constants (twoviewstereo.cpp:69-71, 378, 390)."""
    m = SrhTwoviewMrfParams()
    lib().srh_twoview_mrf_params_defaults(C.byref(m))
    for k, v in kw.items():
        k = "lambda_" if k == "lambda" else k
        if not hasattr(m, k):
            raise AttributeError(k)
        setattr(m, k, v)
    return m


def twoview_sgm_params(**kw):
    """srh_twoview_sgm_params with its defaults (smooth_exp 1, smooth_max 2, lambda 0.25, path_mask 0xFF)."""
    m = SrhTwoviewSgmParams()
    lib().srh_twoview_sgm_params_defaults(C.byref(m))
    for k, v in kw.items():
        k = "lambda_" if k == "lambda" else k
        if not hasattr(m, k):
            raise AttributeError(k)
        setattr(m, k, v)
    return m


def mvs_sgm_params(**kw):
    """srh_mvs_sgm_params with its defaults (beta 1, lambda 1, phi_u 0.5, psi_u 0.002, path_mask 0xFF)."""
    m = SrhMvsSgmParams()
    lib().srh_mvs_sgm_params_defaults(C.byref(m))
    for k, v in kw.items():
        k = "lambda_" if k == "lambda" else k
        if not hasattr(m, k):
            raise AttributeError(k)
        setattr(m, k, v)
    return m


def _sgm_info(info):
    return dict(paths=info.paths, energy=info.energy)


def fuse_params(**kw):
    """srh_fuse_params with its defaults (dist_threshold 0, normal_depth_gap 0, min_views 2, flags 0)."""
    f = FuseParams()
    lib().srh_fuse_params_defaults(C.byref(f))
    for k, v in kw.items():
        if not hasattr(f, k):
            raise AttributeError(k)
        setattr(f, k, v)
    return f


def rectify_params(**kw):
    """srh_rectify_params with its defaults (focal 0 = auto, cx_a, cx_b, cy NaN = auto, out_w, out_h 0 = view a's size,
    flags 0)."""
    r = RectifyParams()
    lib().srh_rectify_params_defaults(C.byref(r))
    for k, v in kw.items():
        if not hasattr(r, k):
            raise AttributeError(k)
        setattr(r, k, v)
    return r


def rectify_cameras(cam_a, cam_b, w, h, image_scale=1.0, r=None):
    """The rectified cameras (ra, rb) of a pair whose scaled images are w x h (srh_rectify_cameras; needs no device)."""
    ra, rb = Camera(), Camera()
    _check(lib().srh_rectify_cameras(C.byref(cam_a), C.byref(cam_b), int(w), int(h), float(image_scale),
                                     C.byref(r) if r is not None else None, C.byref(ra), C.byref(rb)))
    return ra, rb


def twoview_row_aligned(cam_a, cam_b):
    """The dense plan's rig test (srh_twoview_row_aligned): (True, fx_bx) or (False, None)."""
    f = C.c_double(0.0)
    yes = lib().srh_twoview_row_aligned(C.byref(cam_a), C.byref(cam_b), C.byref(f))
    return (True, f.value) if yes else (False, None)


def _mrf_info(info):
    return dict(iterations=info.iterations, energy_initial=info.energy_initial, energy_final=info.energy_final)


def params_mvs(**kw):
    p = Params()
    lib().srh_params_mvs_defaults(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def camera_from_krt(K, R, t, dist=None, plane_normal=None, plane_dist=0.0, refr_index=1.0):
    """Camera::set(K,R,t) + distortion + refractive interface -> srh_camera snapshot."""
    cam = Camera()
    K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    d = None if dist is None else np.ascontiguousarray(dist, dtype=np.float64).reshape(5)
    n = None if plane_normal is None else np.ascontiguousarray(plane_normal, dtype=np.float64).reshape(3)
    _check(lib().srh_camera_from_krt(_dptr(K), _dptr(R), _dptr(t),
                                     _dptr(d) if d is not None else None,
                                     _dptr(n) if n is not None else None,
                                     plane_dist, refr_index, C.byref(cam)))
    return cam


def camera_from_p(P, dist=None, plane_normal=None, plane_dist=0.0, refr_index=1.0):
    """Camera::setP (3x4 projection matrix, the project-file path) -> srh_camera snapshot."""
    cam = Camera()
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(12)
    d = None if dist is None else np.ascontiguousarray(dist, dtype=np.float64).reshape(5)
    n = None if plane_normal is None else np.ascontiguousarray(plane_normal, dtype=np.float64).reshape(3)
    _check(lib().srh_camera_from_p(_dptr(P), _dptr(d) if d is not None else None,
                                   _dptr(n) if n is not None else None, plane_dist, refr_index, C.byref(cam)))
    return cam


def mvs_neighbours(cams, p):
    n = len(cams)
    arr = (Camera * n)(*cams)
    neigh = np.full((n, max(1, p.num_neighbours)), -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    _check(lib().srh_mvs_neighbours(n, arr, C.byref(p), neigh.ctypes.data_as(c_int32_p),
                                    cnt.ctypes.data_as(c_int32_p)))
    return [[int(v) for v in neigh[i, :cnt[i]]] for i in range(n)]


def comm_version():
    """NCCL_VERSION_CODE of the librccl the library loads (ncclGetVersion), 0 when there is none: srh_comm_version."""
    return int(lib().srh_comm_version())


def comm_set_timeout_ms(ms):
    _check(lib().srh_comm_set_timeout_ms(int(ms)))


def cert_bound(p, mvs=False):
    """srh_cert_bound: the constants of the certified arithmetic's error bound for these parameters, as a dict."""
    ci = CertInfo()
    _check(lib().srh_cert_bound(C.byref(p), 1 if mvs else 0, C.byref(ci)))
    return {k: getattr(ci, k) for k, _ in CertInfo._fields_}


def tscan_bound(ref_cam, oth_cam, p, template_xy, xy):
    """srh_tscan_bound: the template scan's per-pixel bound for pixel xy of the reference view against the template pixel
    template_xy (host arithmetic, no GPU), as a dict: E, eU, eU_template, dyU, the three rooms, pixel_ok, template_ok, passes."""
    L = lib()
    L.srh_tscan_bound.argtypes = [C.POINTER(Camera), C.POINTER(Camera), C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(TscanBoundInfo)]
    bi = TscanBoundInfo()
    _check(L.srh_tscan_bound(C.byref(ref_cam), C.byref(oth_cam), C.byref(p), int(template_xy[0]), int(template_xy[1]),
                             int(xy[0]), int(xy[1]), C.byref(bi)))
    return {k: getattr(bi, k) for k, _ in TscanBoundInfo._fields_ if k != "pad_"}


def cert_sigma3(p, sum2, mvs=False):
    """srh_cert_sigma3: the smallest sum3 for which a candidate of a pixel with this sum2 is certified (+inf: none)."""
    return float(lib().srh_cert_sigma3(C.byref(p), 1 if mvs else 0, float(sum2)))


def hw_queues_requested():
    """Hardware queues the HIP runtime was asked for (GPU_MAX_HW_QUEUES, else the runtime's default 4): srh_hw_queues_requested."""
    return int(lib().srh_hw_queues_requested())


def device_count():
    n = C.c_int(0)
    _check(lib().srh_device_count(C.byref(n)))
    return n.value


def scaled_size(src_w, src_h, image_scale, mode=SCALE_SMOOTH):
    """(w, h) QImage::scaledToWidth((int)(src_w*image_scale), mode) gives (srh_scaled_size; no device).  A shape the library
    does not scale raises StereoHipError with .code SRH_E_INVALID (-1) or SRH_E_UNSUPPORTED (-5)."""
    w, h = C.c_int(0), C.c_int(0)
    _check(lib().srh_scaled_size(int(src_w), int(src_h), float(image_scale), int(mode), C.byref(w), C.byref(h)))
    return w.value, h.value


def _rgba_arg(rgba, what="rgba"):
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError("%s must be HxWx4 uint8" % what)
    return rgba


def _torch_runtime_first():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64; this library links the
    system ROCm.  Both can live in one process, but the bundled runtime must attach to the GPU first
    (the other order leaves torch with "No HIP GPUs are available").  So when the process has torch
    loaded, its runtime is initialised before the first srh_create; torch itself is never required."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and not torch.cuda.is_initialized():
        torch.cuda.init()


def build_id():
    """Hash of the sources the loaded library was built from (srh_build_id)."""
    return lib().srh_build_id().decode()


class Context:
    """One srh_context bound to one GPU."""

    def __init__(self, device=0):
        _torch_runtime_first()
        self._h = C.c_void_p()
        _check(lib().srh_create(device, C.byref(self._h)))
        self._keep = []
        self._comm_ranks = 0

    def close(self):
        if self._h:
            lib().srh_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing
    def set_stream(self, stream_ptr):
        _check(lib().srh_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_hooks(self, cancel_flag=None, progress=None):
        """cancel_flag: ctypes.c_int; progress: callable(step, stage_str)."""
        cb = PROGRESS_FN(lambda step, stage, user: progress(step, stage.decode())) if progress else PROGRESS_FN()
        self._keep = [cb, cancel_flag]
        _check(lib().srh_set_hooks(self._h, C.byref(cancel_flag) if cancel_flag is not None else None, cb, None))

    def set_option(self, name, value):
        _check(lib().srh_set_option(self._h, name.encode(), int(value)))

    def synchronize(self):
        _check(lib().srh_synchronize(self._h))

    # -- views
    def upload_view(self, slot, rgba, mask, cam):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("rgba must be HxWx4 uint8")
        h, w = rgba.shape[:2]
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (h, w):
                raise ValueError("mask must be HxW uint8")
        _check(lib().srh_view_upload(self._h, slot, w, h, rgba.ctypes.data_as(c_uint8_p),
                                     m.ctypes.data_as(c_uint8_p) if m is not None else None, C.byref(cam)))

    def scale_image(self, rgba, has_alpha, image_scale, mode=SCALE_SMOOTH):
        """rgba (HxWx4, file resolution) scaled on the device as Qt scales it (srh_image_scale): the scaled HxWx4 bytes."""
        rgba = _rgba_arg(rgba)
        h, w = rgba.shape[:2]
        dw, dh = scaled_size(w, h, image_scale, mode)
        out = np.empty((dh, dw, 4), dtype=np.uint8)
        _check(lib().srh_image_scale(self._h, rgba.ctypes.data_as(c_uint8_p), w, h, int(bool(has_alpha)), float(image_scale),
                                     int(mode), out.ctypes.data_as(c_uint8_p), None, None))
        return out

    def upload_view_scaled(self, slot, rgba, has_alpha, image_scale, cam, mask_rule=MASK_NONE, mask_rgba=None, mask_has_alpha=False):
        """The view at file resolution: scaled on the device, mask by mask_rule (MASK_ALPHA_FAST: MultiViewStereo's rule;
        MASK_IMAGE_SMOOTH with mask_rgba: TwoViewStereo's), then as upload_view of the scaled bytes (srh_view_upload_scaled)."""
        rgba = _rgba_arg(rgba)
        h, w = rgba.shape[:2]
        m, mw, mh = None, 0, 0
        if mask_rgba is not None:
            m = _rgba_arg(mask_rgba, "mask_rgba")
            mh, mw = m.shape[:2]
        _check(lib().srh_view_upload_scaled(self._h, slot, w, h, rgba.ctypes.data_as(c_uint8_p), int(bool(has_alpha)),
                                            m.ctypes.data_as(c_uint8_p) if m is not None else None, mw, mh, int(bool(mask_has_alpha)),
                                            float(image_scale), int(mask_rule), C.byref(cam)))

    def download_view_image(self, slot):
        """(rgba HxWx4, mask HxW) as the slot holds them (srh_view_image_download)."""
        w, h = self.view_size(slot)
        rgba = np.empty((h, w, 4), dtype=np.uint8)
        mask = np.empty((h, w), dtype=np.uint8)
        _check(lib().srh_view_image_download(self._h, slot, rgba.ctypes.data_as(c_uint8_p), mask.ctypes.data_as(c_uint8_p)))
        return rgba, mask

    def view_size(self, slot):
        w, h = C.c_int(0), C.c_int(0)
        _check(lib().srh_view_size(self._h, slot, C.byref(w), C.byref(h)))
        return w.value, h.value

    def download_depth(self, slot):
        w, h = self.view_size(slot)
        out = np.empty((h, w), dtype=np.float64)
        _check(lib().srh_view_depth_download(self._h, slot, _dptr(out)))
        return out

    def view_census(self, slot):
        """The 9x7 census signatures of a view -> (h, w) uint64 (srh_view_census): bit (dy + 3)*9 + (dx + 4) is set iff the
        neighbour lies inside the image and is darker than the centre; what COST_CENSUS matches on."""
        w, h = self.view_size(slot)
        out = np.empty((h, w), dtype=np.uint64)
        _check(lib().srh_view_census(self._h, slot, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def upload_depth(self, slot, depth):
        w, h = self.view_size(slot)
        d = np.ascontiguousarray(depth, dtype=np.float64)
        if d.shape != (h, w):
            raise ValueError("depth must be %dx%d" % (h, w))
        _check(lib().srh_view_depth_upload(self._h, slot, _dptr(d)))

    def depth_device_ptr(self, slot):
        p = C.c_void_p()
        _check(lib().srh_view_depth_device_ptr(self._h, slot, C.byref(p)))
        return p.value

    def wta_outputs_state(self, slot):
        """(flags, oth_slot): the WTA_* planes the slot holds from its last WTA pass as the reference view (0: none) and the
        other view of that pass (srh_view_wta_outputs_state)."""
        f, o = C.c_int(0), C.c_int(-1)
        _check(lib().srh_view_wta_outputs_state(self._h, slot, C.byref(f), C.byref(o)))
        return f.value, o.value

    def wta_outputs(self, slot, costs=None):
        """The by-products of the slot's last WTA pass (option "wta_outputs"): dict(win_xy (h, w, 2) int32, runner_xy
        (h, w, 2) int32, min_cost (h, w), second_cost (h, w)); (-1, -1) / +inf = none.  costs: None = the cost planes when
        they were kept (else absent from the dict), True = ask for them (an error when only the winners were kept)."""
        w, h = self.view_size(slot)
        if costs is None:
            costs = bool(self.wta_outputs_state(slot)[0] & WTA_COSTS)
        out = {"win_xy": np.empty((h, w, 2), dtype=np.int32), "runner_xy": np.empty((h, w, 2), dtype=np.int32)}
        if costs:
            out["min_cost"] = np.empty((h, w), dtype=np.float64)
            out["second_cost"] = np.empty((h, w), dtype=np.float64)
        _check(lib().srh_view_wta_outputs(self._h, slot, out["win_xy"].ctypes.data_as(c_int32_p),
                                          out["runner_xy"].ctypes.data_as(c_int32_p),
                                          _dptr(out["min_cost"]) if costs else None, _dptr(out["second_cost"]) if costs else None))
        return out

    def wta_outputs_device(self, slot, costs=True):
        """Device addresses (win_xy, runner_xy, min_cost, second_cost) of the slot's planes (srh_view_wta_outputs_device)."""
        p = [C.c_void_p() for _ in range(4)]
        _check(lib().srh_view_wta_outputs_device(self._h, slot, C.byref(p[0]), C.byref(p[1]),
                                                 C.byref(p[2]) if costs else None, C.byref(p[3]) if costs else None))
        return tuple(q.value for q in p)

    def subpixel(self, slot):
        """What option "subpixel" did in the slot's last WTA pass as the reference view (srh_view_subpixel): dict(delta
        (h, w), 0 where the pixel is not refined; neigh_xy (h, w, 4) int32 = (n-.x, n-.y, n+.x, n+.y), (-1, -1) = none;
        cls (h, w) uint8 of SUBPX_*)."""
        w, h = self.view_size(slot)
        out = {"delta": np.empty((h, w), dtype=np.float64), "neigh_xy": np.empty((h, w, 4), dtype=np.int32),
               "cls": np.empty((h, w), dtype=np.uint8)}
        _check(lib().srh_view_subpixel(self._h, slot, _dptr(out["delta"]), out["neigh_xy"].ctypes.data_as(c_int32_p),
                                       out["cls"].ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def subpixel_device(self, slot):
        """Device addresses (delta, neigh_xy, cls) of the slot's sub-pixel planes (srh_view_subpixel_device)."""
        p = [C.c_void_p() for _ in range(3)]
        _check(lib().srh_view_subpixel_device(self._h, slot, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])))
        return tuple(q.value for q in p)

    def subpixel_info(self, slot):
        """dict(n_class = pixels per SUBPX_* class (5 ints), n_moved = refined pixels with delta != 0) of the slot's
        planes (srh_view_subpixel_info)."""
        i = SubpixelInfo()
        _check(lib().srh_view_subpixel_info(self._h, slot, C.byref(i)))
        return {"n_class": [int(v) for v in i.n_class], "n_moved": int(i.n_moved)}

    def copy_depth_to_device(self, slot, dst_dev_ptr, dst_bytes):
        _check(lib().srh_view_depth_copy_to_device(self._h, slot, C.c_void_p(dst_dev_ptr), C.c_size_t(dst_bytes)))

    def copy_depth_from_device(self, slot, src_dev_ptr, src_bytes):
        _check(lib().srh_view_depth_copy_from_device(self._h, slot, C.c_void_p(src_dev_ptr), C.c_size_t(src_bytes)))

    # -- TwoViewStereo
    def twoview_wta(self, ref_slot, oth_slot, p, y0=0, y1=0):
        _check(lib().srh_twoview_wta(self._h, ref_slot, oth_slot, C.byref(p), y0, y1))

    def twoview_cross_check(self, left_slot, right_slot, p):
        _check(lib().srh_twoview_cross_check(self._h, left_slot, right_slot, C.byref(p)))

    def twoview_compute(self, left_slot, right_slot, p):
        w, h = self.view_size(left_slot)
        dl = np.empty((h, w), dtype=np.float64)
        dr = np.empty((h, w), dtype=np.float64)
        _check(lib().srh_twoview_compute(self._h, left_slot, right_slot, C.byref(p), _dptr(dl), _dptr(dr)))
        return dl, dr

    def debug_exp(self, x):
        """srh_debug_exp -> (the geodesic kernels' exp sequence, the device library's exp) of the arguments x."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        a, b = np.empty_like(x), np.empty_like(x)
        _check(lib().srh_debug_exp(self._h, _dptr(x), x.size, _dptr(a), _dptr(b)))
        return a, b

    def twoview_compute_device(self, left_slot, right_slot, p):
        """srh_twoview_compute without host outputs: both passes + cross-check, the maps stay in the slots' device memory."""
        _check(lib().srh_twoview_compute(self._h, left_slot, right_slot, C.byref(p), None, None))

    # -- MultiViewStereo
    def twoview_cost_rows(self, ref, oth, p, y0, y1, form, raw=False):
        """srh_twoview_cost_rows (diagnostic) -> (cost (rows, w, cstride) float64 with cost[r, x, k] the cost of column
        lo + k, range (rows, w, 2) int32, used_strip_kernel).  form: 0 the reference's arithmetic, 3 / 5 the certified
        forms, 1 fused unchecked, 2 the single-precision kernel in the form of option "f32_form" (per tile:
        used_strip_kernel is False; raw is ignored).  Under set_option("cost", COST_SAD) the rows are cost_sad's and
        need set_option("sad_dense", 1) and form 0 (anything else raises); under COST_CENSUS they are the census cost's and
        need set_option("census_dense", 1) and form 0 likewise; an entry no kernel wrote is a NaN with all bits set."""
        w, h = self.view_size(ref)
        cs, us = C.c_int(0), C.c_int(0)
        _check(lib().srh_twoview_cost_rows(self._h, ref, oth, C.byref(p), y0, y1, form, 1 if raw else 0, None, 0, None, C.byref(cs), C.byref(us)))
        rows, tiles = y1 - y0, (w + 31) // 32
        buf = np.empty((rows, tiles, cs.value, 32), dtype=np.float64)
        rng = np.empty((rows, w, 2), dtype=np.int32)
        _check(lib().srh_twoview_cost_rows(self._h, ref, oth, C.byref(p), y0, y1, form, 1 if raw else 0, _dptr(buf), buf.size,
                                           rng.ctypes.data_as(c_int32_p), C.byref(cs), C.byref(us)))
        cost = np.ascontiguousarray(buf.transpose(0, 1, 3, 2)).reshape(rows, tiles * 32, cs.value)[:, :w]
        return cost, rng, bool(us.value)

    def mvs_initial_estimate(self, view_slot, neigh_slots, p, y0=0, y1=0, peaks_dev=None):
        ng = np.ascontiguousarray(neigh_slots, dtype=np.int32)
        _check(lib().srh_mvs_initial_estimate(self._h, view_slot, ng.ctypes.data_as(c_int32_p), len(ng),
                                              C.byref(p), y0, y1, C.c_void_p(peaks_dev) if peaks_dev else None))

    def mvs_view_subpixel(self, view_slot, neigh_slots, p, want_planes=False):
        """Sub-pixel depth for the slot's finished depth map (srh_mvs_view_subpixel): it refines whatever the slot holds, so
        call it once per estimate, with the estimate's neighbour list.  -> dict(n_class = pixels per SUBPX_* class (6
        ints, SUBPX_NO_WINNER last), n_moved, n_fallback); with want_planes also delta (h, w), win (h, w, 3) int32 =
        (index into neigh_slots, cx, cy), neigh_xy (h, w, 4) int32 and cls (h, w) uint8."""
        ng = np.ascontiguousarray(neigh_slots, dtype=np.int32)
        i = MvsSubpixelInfo()
        out = {}
        if want_planes:
            w, h = self.view_size(view_slot)
            out = {"delta": np.empty((h, w), dtype=np.float64), "win": np.empty((h, w, 3), dtype=np.int32),
                   "neigh_xy": np.empty((h, w, 4), dtype=np.int32), "cls": np.empty((h, w), dtype=np.uint8)}
        _check(lib().srh_mvs_view_subpixel(self._h, view_slot, ng.ctypes.data_as(c_int32_p), len(ng), C.byref(p), C.byref(i),
                                           _dptr(out["delta"]) if want_planes else None,
                                           out["win"].ctypes.data_as(c_int32_p) if want_planes else None,
                                           out["neigh_xy"].ctypes.data_as(c_int32_p) if want_planes else None,
                                           out["cls"].ctypes.data_as(C.POINTER(C.c_uint8)) if want_planes else None))
        out.update(n_class=[int(v) for v in i.n_class], n_moved=int(i.n_moved), n_fallback=int(i.n_fallback))
        return out

    def mvs_cross_check(self, slots, view_index, p):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        _check(lib().srh_mvs_cross_check(self._h, s.ctypes.data_as(c_int32_p), len(s), view_index, C.byref(p)))

    def point_cloud(self, slot, p):
        """-> dict(xyz (h,w,3) float64 with NaN where there is no point, rgb (h,w,3) uint8, valid (h,w) uint8,
        n_points, n_masked, n_finite): srh_view_point_cloud."""
        w, h = self.view_size(slot)
        xyz = np.empty((h, w, 3), dtype=np.float64)
        rgb = np.empty((h, w, 3), dtype=np.uint8)
        valid = np.empty((h, w), dtype=np.uint8)
        n = (C.c_int64 * 3)()
        _check(lib().srh_view_point_cloud(self._h, slot, C.byref(p), _dptr(xyz), rgb.ctypes.data_as(c_uint8_p),
                                          valid.ctypes.data_as(c_uint8_p), C.cast(C.byref(n, 0), C.c_void_p),
                                          C.cast(C.byref(n, 8), C.c_void_p), C.cast(C.byref(n, 16), C.c_void_p)))
        return dict(xyz=xyz, rgb=rgb, valid=valid, n_points=int(n[0]), n_masked=int(n[1]), n_finite=int(n[2]))

    def mvs_fuse(self, slots, p, f=None):
        """The depth maps of the listed slots fused into one oriented cloud (srh_mvs_fuse) -> dict(xyz (n,3) float64,
        normals (n,3) float64, rgb (n,3) uint8, nviews (n,) uint8, flags (n,) uint8 (bit 0: the normal comes from the
        surface), src (n,2) int32 (index into `slots`, pixel index), n_points, n_candidates, n_claimed, n_unsupported,
        n_normals)."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        info = FuseInfo()
        _check(lib().srh_mvs_fuse(self._h, s.ctypes.data_as(c_int32_p), len(s), C.byref(p),
                                  C.byref(f) if f is not None else None, C.byref(info)))
        out = self.mvs_fused_download(0, self.mvs_fused_count())
        out.update({k: int(getattr(info, k)) for k, _ in FuseInfo._fields_})
        return out

    def mvs_fused_count(self):
        n = C.c_int64(0)
        _check(lib().srh_mvs_fused_count(self._h, C.byref(n)))
        return int(n.value)

    def mvs_fused_download(self, first, count):
        """Points [first, first + count) of the last srh_mvs_fuse -> dict of arrays (see mvs_fuse)."""
        k = max(int(count), 0)
        out = dict(xyz=np.empty((k, 3), np.float64), normals=np.empty((k, 3), np.float64), rgb=np.empty((k, 3), np.uint8),
                   nviews=np.empty(k, np.uint8), flags=np.empty(k, np.uint8), src=np.empty((k, 2), np.int32))
        _check(lib().srh_mvs_fused_download(self._h, first, count, _dptr(out["xyz"]), _dptr(out["normals"]),
                                            out["rgb"].ctypes.data_as(c_uint8_p), out["nviews"].ctypes.data_as(c_uint8_p),
                                            out["flags"].ctypes.data_as(c_uint8_p), out["src"].ctypes.data_as(c_int32_p)))
        return out

    def mvs_fused_device(self):
        """Device addresses of the fused cloud's arrays -> dict(xyz, normals, rgb, nviews, flags, src) of ints (0: empty)."""
        ptrs = [C.c_void_p() for _ in range(6)]
        _check(lib().srh_mvs_fused_device(self._h, *[C.byref(q) for q in ptrs]))
        return dict(zip(("xyz", "normals", "rgb", "nviews", "flags", "src"), [q.value or 0 for q in ptrs]))

    def filter_invalid(self, slot, p, flags=FILTER_GAPS | FILTER_MEDIAN, gap_width=2):
        """TwoViewStereo::filterInvalidPixels on the slot's depth map, in place (srh_view_filter_invalid)
        -> dict(holes, gap_filled, median_filled, replayed)."""
        info = FilterInfo()
        _check(lib().srh_view_filter_invalid(self._h, slot, C.byref(p), flags, gap_width, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in FilterInfo._fields_}

    def filter_speckles(self, slot, p, min_size, max_diff=0.0, flags=0, want_labels=False):
        """The speckle filter on the slot's depth map, in place (srh_view_filter_speckles): the 4-connected components of
        valid pixels whose depths differ by at most max_diff (<= 0: two depth steps of p), those smaller than min_size
        overwritten with +INF (SPECKLE_TO_NAN: NaN) -> dict(valid, components, removed_components, removed_pixels, largest);
        want_labels: (that dict, labels (h, w) int32: the components' labels before the removal, -1 = not valid)."""
        s = SpeckleParams(float(max_diff), int(min_size), int(flags))
        info = SpeckleInfo()
        labels = None
        if want_labels:
            w, h = self.view_size(slot)
            labels = np.empty((h, w), dtype=np.int32)
        _check(lib().srh_view_filter_speckles(self._h, slot, C.byref(p), C.byref(s), C.byref(info),
                                              labels.ctypes.data_as(c_int32_p) if want_labels else None))
        out = {k: int(getattr(info, k)) for k, _ in SpeckleInfo._fields_}
        return (out, labels) if want_labels else out

    def twoview_rectify(self, src_a, src_b, dst_a, dst_b, p, r=None):
        """The views of src_a, src_b warped onto the rectified cameras into dst_a, dst_b (srh_twoview_rectify; a destination
        may be a source) -> dict(angle_a, angle_b, fx_bx, white_a, white_b)."""
        info = RectifyInfo()
        _check(lib().srh_twoview_rectify(self._h, src_a, src_b, dst_a, dst_b, C.byref(p), C.byref(r) if r is not None else None,
                                         C.byref(info)))
        return {k: getattr(info, k) for k, _ in RectifyInfo._fields_}

    def rectify_map(self, src_slot, rect_cam, out_w, out_h, image_scale=1.0):
        """(out_h, out_w, 2): where every pixel of a rectified view with camera rect_cam reads slot src_slot's image, (u, v)
        with pixel centres at integers, NaN where it reads nothing (srh_view_rectify_map)."""
        uv = np.empty((int(out_h), int(out_w), 2), dtype=np.float64)
        _check(lib().srh_view_rectify_map(self._h, src_slot, C.byref(rect_cam), int(out_w), int(out_h), float(image_scale), _dptr(uv)))
        return uv

    def depth_unrectify(self, rect_slot, dst_slot, p, want_index=False):
        """The depth map of the rectified view rect_slot into the depth map of dst_slot, the view the user handed in
        (srh_view_depth_unrectify); want_index: returns (h, w) int32, the rectified pixel every pixel read (-1: none)."""
        idx = None
        if want_index:
            w, h = self.view_size(dst_slot)
            idx = np.empty((h, w), dtype=np.int32)
        _check(lib().srh_view_depth_unrectify(self._h, rect_slot, dst_slot, C.byref(p),
                                              idx.ctypes.data_as(c_int32_p) if idx is not None else None))
        return idx

    def twoview_pair_costs(self, ref, oth, p, xy, kind=COST_SAD):
        """cost_sad (kind COST_SAD), cost_ncc (COST_NCC) or the census cost (COST_CENSUS) of arbitrary pairs: xy (n, 4) int rows (x1, y1, x2, y2), the
        support window of (x1, y1) in view `ref` -> (n,) float64 (srh_twoview_pair_costs)."""
        a = np.ascontiguousarray(np.asarray(xy, dtype=np.int32).reshape(-1, 4))
        out = np.empty(a.shape[0], np.float64)
        _check(lib().srh_twoview_pair_costs(self._h, ref, oth, C.byref(p), kind, a.shape[0],
                                            a.ctypes.data_as(c_int32_p), out.ctypes.data_as(c_double_p)))
        return out

    def mvs_mrf_estimate(self, view_slot, top_k, peaks_dev, m=None):
        """MRF branch of computeInitialEstimate on the device peaks buffer -> dict(iterations, energy_initial, energy_final)."""
        m = m if m is not None else mrf_params()
        info = SrhMrfInfo()
        _check(lib().srh_mvs_mrf_estimate(self._h, view_slot, top_k, C.c_void_p(peaks_dev), C.byref(m), C.byref(info)))
        return dict(iterations=info.iterations, energy_initial=info.energy_initial, energy_final=info.energy_final)

    def mvs_initial_estimate_mrf(self, view_slot, neigh_slots, p, m=None):
        """computeInitialEstimate of a CONFIG+=mrf build: peaks, then TRW-S on them."""
        m = m if m is not None else mrf_params()
        info = SrhMrfInfo()
        nb = np.ascontiguousarray(neigh_slots, dtype=np.int32)
        _check(lib().srh_mvs_initial_estimate_mrf(self._h, view_slot, nb.ctypes.data_as(c_int32_p), len(nb), C.byref(p),
                                                  C.byref(m), C.byref(info)))
        return dict(iterations=info.iterations, energy_initial=info.energy_initial, energy_final=info.energy_final)

    def mvs_initial_estimate_peaks(self, view_slot, neigh_slots, p):
        """Initial estimate of one view, its top-K peaks kept in the context for mvs_mrf_estimate_views."""
        nb = np.ascontiguousarray(neigh_slots, dtype=np.int32)
        _check(lib().srh_mvs_initial_estimate_peaks(self._h, view_slot, nb.ctypes.data_as(c_int32_p), len(nb), C.byref(p)))

    def mvs_mrf_estimate_views(self, view_slots, m=None):
        """MRF stage of several views side by side -> list of dict(iterations, energy_initial, energy_final)."""
        m = m if m is not None else mrf_params()
        sl = np.ascontiguousarray(view_slots, dtype=np.int32)
        infos = (SrhMrfInfo * len(sl))()
        _check(lib().srh_mvs_mrf_estimate_views(self._h, sl.ctypes.data_as(c_int32_p), len(sl), C.byref(m), infos))
        return [dict(iterations=i.iterations, energy_initial=i.energy_initial, energy_final=i.energy_final) for i in infos]

    def mvs_mrf_state(self, w, h, top_k):
        """(labels (h,w) int32, data_costs (h,w,K+1), messages (h,w,2,K+1)) of the last MRF run."""
        labels = np.zeros((h, w), dtype=np.int32)
        D = np.zeros((h, w, top_k + 1), dtype=np.float64)
        M = np.zeros((h, w, 2, top_k + 1), dtype=np.float64)
        _check(lib().srh_mvs_mrf_state(self._h, w, h, top_k, labels.ctypes.data_as(c_int32_p), _dptr(D), _dptr(M)))
        return labels, D, M

    def mvs_mrf_dims(self):
        """(w, h, top_k) of the single-view MRF run whose state mvs_mrf_state reports."""
        w, h, k = C.c_int(), C.c_int(), C.c_int()
        _check(lib().srh_mvs_mrf_dims(self._h, C.byref(w), C.byref(h), C.byref(k)))
        return w.value, h.value, k.value

    # -- MultiViewStereo, semi-global aggregation over the peak labels
    def mvs_sgm_estimate(self, view_slot, top_k, peaks_dev, m=None):
        """The aggregation on the device peaks buffer; writes the slot's depth map -> dict(paths, energy)."""
        m = m if m is not None else mvs_sgm_params()
        info = SrhSgmInfo()
        _check(lib().srh_mvs_sgm_estimate(self._h, view_slot, top_k, C.c_void_p(peaks_dev), C.byref(m), C.byref(info)))
        return _sgm_info(info)

    def mvs_initial_estimate_sgm(self, view_slot, neigh_slots, p, m=None):
        """Peaks of the view, then the aggregation on them -> dict(paths, energy)."""
        m = m if m is not None else mvs_sgm_params()
        info = SrhSgmInfo()
        nb = np.ascontiguousarray(neigh_slots, dtype=np.int32)
        _check(lib().srh_mvs_initial_estimate_sgm(self._h, view_slot, nb.ctypes.data_as(c_int32_p), len(nb), C.byref(p),
                                                  C.byref(m), C.byref(info)))
        return _sgm_info(info)

    def mvs_sgm_estimate_views(self, view_slots, m=None):
        """The aggregation of several views side by side (peaks kept by mvs_initial_estimate_peaks) -> list of dict(paths, energy)."""
        m = m if m is not None else mvs_sgm_params()
        sl = np.ascontiguousarray(view_slots, dtype=np.int32)
        infos = (SrhSgmInfo * len(sl))()
        _check(lib().srh_mvs_sgm_estimate_views(self._h, sl.ctypes.data_as(c_int32_p), len(sl), C.byref(m), infos))
        return [_sgm_info(i) for i in infos]

    def mvs_sgm_state(self, w, h, top_k):
        """(labels (h,w) int32, data_costs (h,w,K+1), sums (h,w,K+1)) of the last single-view aggregation."""
        labels = np.zeros((h, w), dtype=np.int32)
        D = np.zeros((h, w, top_k + 1), dtype=np.float64)
        S = np.zeros((h, w, top_k + 1), dtype=np.float64)
        _check(lib().srh_mvs_sgm_state(self._h, w, h, top_k, labels.ctypes.data_as(c_int32_p), _dptr(D), _dptr(S)))
        return labels, D, S

    def mvs_sgm_dims(self):
        """(w, h, top_k) of the single-view aggregation whose state mvs_sgm_state reports."""
        w, h, k = C.c_int(), C.c_int(), C.c_int()
        _check(lib().srh_mvs_sgm_dims(self._h, C.byref(w), C.byref(h), C.byref(k)))
        return w.value, h.value, k.value

    # -- TwoViewStereo, MRF stage
    def twoview_label_costs(self, ref_slot, oth_slot, p, y0=0, y1=0, want_pixels=True):
        """The label cost volume of rows [y0, y1) (y1 <= 0: all) -> (costs (rows, w, D) float64, pixels (rows, w, D, 2) int32
        or None): srh_twoview_label_costs.  A label without a pixel holds LABEL_PIXEL_NONE."""
        w, h = self.view_size(ref_slot)
        rows = (y1 if y1 > 0 else h) - y0
        D = p.num_depth_levels
        cost = np.empty((max(rows, 0), w, D), dtype=np.float64)
        pix = np.empty((max(rows, 0), w, D, 2), dtype=np.int32) if want_pixels else None
        _check(lib().srh_twoview_label_costs(self._h, ref_slot, oth_slot, C.byref(p), y0, y1, _dptr(cost),
                                             pix.ctypes.data_as(c_int32_p) if want_pixels else None))
        return cost, pix

    def twoview_mrf_optimize(self, view_slot, p, L, costs_dev, m=None):
        """TRW-S on a device volume (w*h*L doubles, [pixel][label]); writes the slot's depth map
        -> dict(iterations, energy_initial, energy_final)."""
        m = m if m is not None else twoview_mrf_params()
        info = SrhMrfInfo()
        _check(lib().srh_twoview_mrf_optimize(self._h, view_slot, C.byref(p), L, C.c_void_p(costs_dev), C.byref(m), C.byref(info)))
        return _mrf_info(info)

    def twoview_mrf(self, ref_slot, oth_slot, p, m=None):
        """One direction of the MRF stage: label costs, optimiser, depth map of ref_slot."""
        m = m if m is not None else twoview_mrf_params()
        info = SrhMrfInfo()
        _check(lib().srh_twoview_mrf(self._h, ref_slot, oth_slot, C.byref(p), C.byref(m), C.byref(info)))
        return _mrf_info(info)

    def twoview_compute_mrf(self, left_slot, right_slot, p, m=None):
        """computeDepthMaps of a USE_MRF build -> (left map, right map, [left info, right info])."""
        m = m if m is not None else twoview_mrf_params()
        w, h = self.view_size(left_slot)
        dl = np.empty((h, w), dtype=np.float64)
        dr = np.empty((h, w), dtype=np.float64)
        infos = (SrhMrfInfo * 2)()
        _check(lib().srh_twoview_compute_mrf(self._h, left_slot, right_slot, C.byref(p), C.byref(m), _dptr(dl), _dptr(dr), infos))
        return dl, dr, [_mrf_info(i) for i in infos]

    def twoview_mrf_state(self, w, h, L, want_costs=False):
        """(labels (h,w) int32, data_costs (h,w,L) or None, messages (h,w,2,L)) of the last single-direction run."""
        labels = np.zeros((h, w), dtype=np.int32)
        D = np.zeros((h, w, L), dtype=np.float64) if want_costs else None
        M = np.zeros((h, w, 2, L), dtype=np.float64)
        _check(lib().srh_twoview_mrf_state(self._h, w, h, L, labels.ctypes.data_as(c_int32_p),
                                           _dptr(D) if want_costs else None, _dptr(M)))
        return labels, D, M

    def twoview_mrf_dims(self):
        """(w, h, L) of the run whose state twoview_mrf_state reports."""
        w, h, k = C.c_int(), C.c_int(), C.c_int()
        _check(lib().srh_twoview_mrf_dims(self._h, C.byref(w), C.byref(h), C.byref(k)))
        return w.value, h.value, k.value

    def twoview_sgm_aggregate(self, view_slot, p, L, costs_dev, m=None):
        """Semi-global aggregation on a device volume (w*h*L doubles, [pixel][label], read only); writes the slot's depth
        map -> dict(paths, energy)."""
        m = m if m is not None else twoview_sgm_params()
        info = SrhSgmInfo()
        _check(lib().srh_twoview_sgm_aggregate(self._h, view_slot, C.byref(p), L, C.c_void_p(costs_dev), C.byref(m), C.byref(info)))
        return _sgm_info(info)

    def twoview_sgm(self, ref_slot, oth_slot, p, m=None):
        """One direction of the pair: label costs, aggregation, depth map of ref_slot."""
        m = m if m is not None else twoview_sgm_params()
        info = SrhSgmInfo()
        _check(lib().srh_twoview_sgm(self._h, ref_slot, oth_slot, C.byref(p), C.byref(m), C.byref(info)))
        return _sgm_info(info)

    def twoview_compute_sgm(self, left_slot, right_slot, p, m=None):
        """Both directions, then the cross-check -> (left map, right map, [left info, right info])."""
        m = m if m is not None else twoview_sgm_params()
        w, h = self.view_size(left_slot)
        dl = np.empty((h, w), dtype=np.float64)
        dr = np.empty((h, w), dtype=np.float64)
        infos = (SrhSgmInfo * 2)()
        _check(lib().srh_twoview_compute_sgm(self._h, left_slot, right_slot, C.byref(p), C.byref(m), _dptr(dl), _dptr(dr), infos))
        return dl, dr, [_sgm_info(i) for i in infos]

    def twoview_sgm_state(self, w, h, L, want_costs=False):
        """(labels (h,w) int32, data_costs (h,w,L) or None, sums (h,w,L)) of the last single-direction run."""
        labels = np.zeros((h, w), dtype=np.int32)
        D = np.zeros((h, w, L), dtype=np.float64) if want_costs else None
        S = np.zeros((h, w, L), dtype=np.float64)
        _check(lib().srh_twoview_sgm_state(self._h, w, h, L, labels.ctypes.data_as(c_int32_p),
                                           _dptr(D) if want_costs else None, _dptr(S)))
        return labels, D, S

    def twoview_sgm_dims(self):
        """(w, h, L) of the run whose state twoview_sgm_state reports."""
        w, h, k = C.c_int(), C.c_int(), C.c_int()
        _check(lib().srh_twoview_sgm_dims(self._h, C.byref(w), C.byref(h), C.byref(k)))
        return w.value, h.value, k.value

    def epipolar_preview(self, ref_slot, oth_slot, min_depth, max_depth, num_depths, xy):
        """The GUI's curve preview (StereoWidget::epipolarLineItem) for the pixels `xy` (n,2) -> list of (k,2) float64."""
        q = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = q.shape[0]
        out = np.zeros((max(n, 1), num_depths, 2), dtype=np.float64)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().srh_epipolar_preview(self._h, ref_slot, oth_slot, C.c_double(min_depth), C.c_double(max_depth),
                                          num_depths, n, _dptr(q), _dptr(out), counts.ctypes.data_as(c_int32_p)))
        return [out[i, :counts[i]].copy() for i in range(n)]

    def refraction_error(self, slot1, slot2, p1, p2):
        """RefractionCalibration::error per pair and totalError -> (errors (n,), total, average)."""
        a = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 2)
        assert a.shape == b.shape
        err = np.zeros(max(len(a), 1), dtype=np.float64)
        tot, avg = C.c_double(0), C.c_double(0)
        _check(lib().srh_refraction_error(self._h, slot1, slot2, len(a), _dptr(a), _dptr(b), _dptr(err), C.byref(tot), C.byref(avg)))
        return err[:len(a)].copy(), tot.value, avg.value

    def epipolar_curves(self, ref_slot, oth_slot, p, xy, mvs=False, max_pts=4096):
        """Candidate pixels of each reference pixel in `xy` (n,2), in the reference's visiting order
        -> list of (len,2) int32 arrays (TwoViewStereo/MultiViewStereo::epipolarCurve)."""
        q = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        n = q.shape[0]
        counts = np.zeros(max(n, 1), dtype=np.int32)
        while True:
            out = np.zeros((max(n, 1), max_pts, 2), dtype=np.int32)
            _check(lib().srh_epipolar_curves(self._h, ref_slot, oth_slot, C.byref(p), int(bool(mvs)), n,
                                             q.ctypes.data_as(c_int32_p), out.ctypes.data_as(c_int32_p), max_pts,
                                             counts.ctypes.data_as(c_int32_p)))
            if n == 0 or counts[:n].max() <= max_pts:
                return [out[i, :counts[i]].copy() for i in range(n)]
            max_pts = int(counts[:n].max())

    # -- multi-GPU exchange (RCCL)
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().srh_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        _check(lib().srh_comm_init(self._h, nranks, rank, C.c_char_p(unique_id)))
        self._comm_ranks = nranks

    def comm_gather_depth(self, slot, root, recv_dev_ptr):
        _check(lib().srh_comm_gather_depth(self._h, slot, root, C.c_void_p(recv_dev_ptr)))

    def comm_allgather_depth(self, slot, recv_dev_ptr):
        _check(lib().srh_comm_allgather_depth(self._h, slot, C.c_void_p(recv_dev_ptr)))

    def comm_allgather_host(self, send):
        """Every rank contributes `send` (float64 host array), every rank receives ranks*len(send) values (host)."""
        a = np.ascontiguousarray(send, dtype=np.float64).reshape(-1)
        out = np.empty(a.size * max(1, self._comm_ranks), dtype=np.float64)
        _check(lib().srh_comm_allgather_host(self._h, a.ctypes.data_as(c_double_p), a.size, out.ctypes.data_as(c_double_p)))
        return out

    def comm_allgather_views(self, view_slots):
        """Sharded MultiViewStereo: every rank contributes the depth maps of its shard of `view_slots`, device to device."""
        sl = np.ascontiguousarray(view_slots, dtype=np.int32)
        _check(lib().srh_comm_allgather_views(self._h, sl.ctypes.data_as(c_int32_p), len(sl)))

    def comm_destroy(self):
        _check(lib().srh_comm_destroy(self._h))

    # -- measurement
    def stats(self):
        s = Stats()
        _check(lib().srh_get_stats(self._h, C.byref(s)))
        return dict(n_pixels=s.n_pixels, n_eval=s.n_eval, n_eval_device=s.n_eval_device,
                    used_dense_path=bool(s.used_dense_path), used_fused_kernel=bool(s.used_fused_kernel),
                    used_strip_kernel=bool(s.used_strip_kernel), band_retries=s.band_retries,
                    n_certified=s.n_certified, n_flagged=s.n_flagged, band_budget_bytes=s.band_budget_bytes,
                    mvs_waves_staged=s.mvs_waves_staged, mvs_waves_listed=s.mvs_waves_listed,
                    scan_tiles_template=s.scan_tiles_template, scan_tiles_walked=s.scan_tiles_walked,
                    scan_tiles_bound=s.scan_tiles_bound)

    def profile_enable(self, on=True):
        _check(lib().srh_profile_enable(self._h, int(on)))

    def profile_reset(self):
        _check(lib().srh_profile_reset(self._h))

    def profile(self):
        buf = C.create_string_buffer(1 << 16)
        _check(lib().srh_profile_dump(self._h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, n = line.split()
            out[name] = (float(ms), int(n))
        return out
