"""ctypes driver of tests/census_restatement.cpp: the CPU restatement of the support-weighted census cost (option "cost" =
COST_CENSUS) and of one WTA pass with it, which the census tests hold the library against.  Compiled with
g++ on first use into a temporary directory, linked to oracle/liboracle.so (sro_weights, sro_unproject,
sro_epipolar_curve, sro_closest_points)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "census_restatement.cpp")

_lib = None
_u64p = C.POINTER(C.c_uint64)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    O.build_oracle()
    out = os.path.join(tempfile.mkdtemp(prefix="census_ref_"), "libcensus_ref.so")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + O.ORACLE_DIR, SRC, "-L" + O.ORACLE_DIR, "-l:liboracle.so",
                           "-Wl,-rpath," + O.ORACLE_DIR, "-o", out])
    L = C.CDLL(out)
    dp, ip, ptr = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER
    L.sr_census_plane.argtypes = [ptr(O.Image), _u64p]
    L.sr_census_plane.restype = None
    L.sr_cost_census.argtypes = [ptr(O.Image), ptr(O.Image), _u64p, _u64p, dp, ptr(O.Params), C.c_int, C.c_int, C.c_int, C.c_int]
    L.sr_cost_census.restype = C.c_double
    L.sr_pair_costs_census.argtypes = [ptr(O.Image), ptr(O.Image), ptr(O.Params), C.c_int, ip, dp]
    L.sr_pair_costs_census.restype = None
    L.sr_twoview_wta_census.argtypes = [ptr(O.Image), ptr(O.Image), ptr(O.Camera), ptr(O.Camera), ptr(O.Params),
                                        C.c_int, C.c_int, dp, dp, ip]
    L.sr_twoview_wta_census.restype = None
    _lib = L
    return L


def _uptr(a):
    return a.ctypes.data_as(_u64p)


def census_plane(img):
    """the signature plane of an OImage -> (h, w) uint64"""
    out = np.empty((img.h, img.w), np.uint64)
    lib().sr_census_plane(C.byref(img.c), _uptr(out))
    return out


def cost_census(left, right, weights, op, x1, y1, x2, y2):
    """the census cost with a given window: left / right = OImage, weights (2R+1, 2R+1), op = sro_params."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    sl, sr = census_plane(left), census_plane(right)
    return lib().sr_cost_census(C.byref(left.c), C.byref(right.c), _uptr(sl), _uptr(sr), O.dptr(w), C.byref(op), x1, y1, x2, y2)


def pair_costs_census(left, right, op, xy):
    """the census cost of pairs (n, 4) = (x1, y1, x2, y2), each with the window of its (x1, y1) (sro_weights)."""
    a = np.ascontiguousarray(np.asarray(xy, dtype=np.int32).reshape(-1, 4))
    out = np.empty(a.shape[0], np.float64)
    lib().sr_pair_costs_census(C.byref(left.c), C.byref(right.c), C.byref(op), a.shape[0], O.iptr(a), O.dptr(out))
    return out


def twoview_wta_census(ref, oth, refcam, othcam, op, y0=0, y1=None, want_cost=False):
    """One census pass of computeCostVolumes; the map is NaN outside rows [y0, y1)."""
    y1 = ref.h if y1 is None else y1
    depth = np.full((ref.h, ref.w), np.nan)
    mc = np.full((ref.h, ref.w), np.inf)
    lib().sr_twoview_wta_census(C.byref(ref.c), C.byref(oth.c), C.byref(refcam), C.byref(othcam), C.byref(op),
                                y0, y1, O.dptr(depth), O.dptr(mc), None)
    return (depth, mc) if want_cost else depth


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def diff_report(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = got.view(np.uint64) != want.view(np.uint64)
    idx = np.argwhere(bad)[:4]
    return "%d of %d differ; first %s: got %s want %s" % (
        bad.sum(), bad.size, idx.tolist(), [got[tuple(i)] for i in idx], [want[tuple(i)] for i in idx])
