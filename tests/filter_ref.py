"""ctypes driver of tests/filter_restatement.cpp: the CPU restatement of TwoViewStereo::filterInvalidPixels /
weightedMedian that the hole-filling tests hold the library against.  Compiled with g++ on first use into a temporary
directory, linked to oracle/liboracle.so (sro_weights)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "filter_restatement.cpp")
CSRC = os.path.join(ROOT, "stereoreconstruction_amd", "csrc")

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    O.build_oracle()
    out = os.path.join(tempfile.mkdtemp(prefix="filter_ref_"), "libfilter_ref.so")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + O.ORACLE_DIR, "-I" + CSRC, SRC, "-L" + O.ORACLE_DIR, "-l:liboracle.so",
                           "-Wl,-rpath," + O.ORACLE_DIR, "-o", out])
    L = C.CDLL(out)
    dp = C.POINTER(C.c_double)
    L.fr_filter.argtypes = [C.POINTER(O.Image), C.POINTER(O.Params), dp, dp, C.c_int, C.c_int]
    L.fr_filter.restype = None
    L.fr_weighted_median.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double]
    L.fr_weighted_median.restype = C.c_double
    L.fr_lib_gap_fill.argtypes = [dp, dp, C.c_int, C.c_int, C.c_int]
    L.fr_lib_gap_fill.restype = None
    L.fr_heap_check.argtypes = [C.c_uint, C.c_int]
    L.fr_heap_check.restype = C.c_int
    _lib = L
    return L


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def oparams(p):
    """srh_params (capi.Params) -> the oracle's sro_params with the fields the filter reads."""
    return O.params_twoview(min_depth=p.min_depth, max_depth=p.max_depth, window_radius=p.window_radius,
                            weight_kind=p.weight_kind, geodesic_iters=p.geodesic_iters,
                            geodesic_sigma=p.geodesic_sigma, geodesic_init=p.geodesic_init,
                            adaptive_color_sigma=p.adaptive_color_sigma)


def filter_map(rgba, mask, depth, op, flags, gap_width=2):
    """The restatement on one map: rgba (h,w,4) u8, mask (h,w) u8 or None, depth (h,w) f64, op = sro_params."""
    img = O.OImage(rgba, mask)
    d = np.ascontiguousarray(depth, dtype=np.float64)
    out = np.empty_like(d)
    lib().fr_filter(C.byref(img.c), C.byref(op), _d(d), _d(out), flags, gap_width)
    return out


def gap_fill(depth, gap_width=2):
    """Gap fill only (no image needed): the restatement's row loop."""
    d = np.ascontiguousarray(np.atleast_2d(depth), dtype=np.float64)
    h, w = d.shape
    rgba = np.zeros((h, w, 4), np.uint8)
    return filter_map(rgba, None, d, O.params_twoview(), 1, gap_width)


def lib_gap_fill(depth, gap_width=2):
    """The library's per-pixel gap fill (srh_filter.hpp compiled for the host)."""
    d = np.ascontiguousarray(np.atleast_2d(depth), dtype=np.float64)
    out = np.empty_like(d)
    lib().fr_lib_gap_fill(_d(d), _d(out), d.shape[1], d.shape[0], gap_width)
    return out


def weighted_median(depths, weights, min_depth, max_depth):
    d = np.ascontiguousarray(depths, dtype=np.float64)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    R = (d.shape[0] - 1) // 2
    return lib().fr_weighted_median(_d(d), _d(w), R, min_depth, max_depth)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
