"""ctypes driver of tests/twoview_mrf_restatement.cpp: the CPU restatement of TwoViewStereo's MRF stage (depthFromLabel,
the fill rule, TRW-S with the truncated-linear term in its direct and its windowed form) that the MRF tests hold the
library against.  Compiled with g++ on first use into a temporary directory; it needs nothing but the C++ library."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "twoview_mrf_restatement.cpp")

DIRECT, WINDOWED = 0, 1
DEFAULTS = dict(smooth_exp=1, smooth_max=2.0, lambda_=0.25, max_iters=50, min_energy_drop=5.0)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    out = os.path.join(tempfile.mkdtemp(prefix="tvmrf_ref_"), "libtvmrf_ref.so")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
    L = C.CDLL(out)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.tvm_depth_from_label.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
    L.tvm_depth_from_label.restype = C.c_double
    L.tvm_fill_value.argtypes = [C.c_int, C.c_double]
    L.tvm_fill_value.restype = C.c_double
    L.tvm_energy.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_double, C.c_double, ip]
    L.tvm_energy.restype = C.c_double
    L.tvm_optimize.argtypes = [C.c_int, C.c_int, C.c_int, dp, bp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int,
                               C.c_double, C.c_double, dp, ip, dp, dp]
    L.tvm_optimize.restype = None
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def depth_from_label(label, D, min_depth, max_depth):
    return lib().tvm_depth_from_label(int(label), int(D), float(min_depth), float(max_depth))


def fill_value(window_radius, bad_ret):
    return lib().tvm_fill_value(int(window_radius), float(bad_ret))


def energy(costs, labels, lambda_=0.25, smooth_max=2.0):
    costs = np.ascontiguousarray(costs, np.float64)
    labels = np.ascontiguousarray(labels, np.int32)
    h, w, L = costs.shape
    return lib().tvm_energy(w, h, L, _dp(costs), lambda_, smooth_max, labels.ctypes.data_as(C.POINTER(C.c_int32)))


def optimize(costs, mask=None, form=WINDOWED, min_depth=1.0, max_depth=2.0, smooth_exp=1, smooth_max=2.0, lambda_=0.25,
             max_iters=50, min_energy_drop=5.0):
    """costs (h, w, L).  Returns dict(labels, messages (h, w, 2, L), depth, iterations, energy_initial, energy_final,
    lower_bound)."""
    assert smooth_exp == 1
    costs = np.ascontiguousarray(costs, np.float64)
    h, w, L = costs.shape
    labels = np.zeros((h, w), np.int32)
    messages = np.zeros((h, w, 2, L))
    depth = np.zeros((h, w))
    info = np.zeros(4)
    mp = None
    if mask is not None:
        mask = np.ascontiguousarray(mask, np.uint8)
        mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    lib().tvm_optimize(w, h, L, _dp(costs), mp, lambda_, smooth_max, max_iters, min_energy_drop, form, min_depth, max_depth,
                       _dp(depth), labels.ctypes.data_as(C.POINTER(C.c_int32)), _dp(messages), _dp(info))
    return dict(labels=labels, messages=messages, depth=depth, iterations=int(info[0]), energy_initial=info[1],
                energy_final=info[2], lower_bound=info[3])
