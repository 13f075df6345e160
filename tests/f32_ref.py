"""ctypes driver of tests/f32_restatement.cpp: the CPU restatement of the single-precision cost kernel of the dense TwoView
plan (srh_dense_f32.hip, "arith" = 2), the same cost in double and the first-order error bound between the two.  Compiled
with g++ on first use into a temporary directory, linked to oracle/liboracle.so."""
import ctypes as C
import os
import subprocess
import tempfile
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "f32_restatement.cpp")
FLAGS = ["-std=c++14", "-O1", "-ffp-contract=off"]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    O.build_oracle()
    out = os.path.join(tempfile.mkdtemp(prefix="f32_ref_"), "libf32_ref.so")
    subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-I" + O.ORACLE_DIR, SRC, "-L" + O.ORACLE_DIR, "-l:liboracle.so",
                                             "-Wl,-rpath," + O.ORACLE_DIR, "-o", out])
    L = C.CDLL(out)
    dp, ip, bp, ptr = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER
    L.f32r_window.argtypes = [dp, dp, dp, C.c_int, ptr(O.Params), dp, dp, ip]
    L.f32r_window.restype = C.c_int
    L.f32r_rows.argtypes = [ptr(O.Image), ptr(O.Image), ptr(O.Params), C.c_int, C.c_int, C.c_int, ip, C.c_int,
                            dp, dp, dp, dp, dp, bp, bp, bp]
    L.f32r_rows.restype = None
    _lib = L
    return L


FAST, GENERAL = 1, 2


def window(w, l, r, op):
    """One window tap by tap (row-major, NaN in l / r = unusable) -> (path, f32[2], B[2], left_out[2])."""
    w, l, r = (np.ascontiguousarray(a, np.float64).ravel() for a in (w, l, r))
    assert w.size == l.size == r.size == (2 * op.window_radius + 1) ** 2
    f, b, lo = np.empty(2), np.empty(2), np.zeros(2, np.int32)
    path = lib().f32r_window(O.dptr(w), O.dptr(l), O.dptr(r), w.size, C.byref(op), O.dptr(f), O.dptr(b), O.iptr(lo))
    return path, f, b, lo


def rows(ref, oth, op, y0, y1, rng, cstride, threads=16):
    """Rows [y0, y1) of ref (an OImage) against oth, the pixels' column ranges rng (rows, w, 2) as
    capi.Context.twoview_cost_rows returns them.  -> f32 (2, rows, w, cstride), f64, B (2, ...), path, noB (2, ...) bool,
    stable (rows, w) bool; entries outside a pixel's range are NaN / 0."""
    L = lib()
    n, w = y1 - y0, ref.w
    rng = np.ascontiguousarray(rng, np.int32)
    assert rng.shape == (n, w, 2)
    f32 = np.full((2, n, w, cstride), np.nan)
    f64 = np.full((n, w, cstride), np.nan)
    B = np.full((2, n, w, cstride), np.nan)
    path = np.zeros((n, w, cstride), np.uint8)
    nob = np.zeros((n, w, cstride), np.uint8)
    stable = np.ones((n, w), np.uint8)

    def band(ab):
        L.f32r_rows(C.byref(ref.c), C.byref(oth.c), C.byref(op), y0, ab[0], ab[1], O.iptr(rng), cstride,
                    O.dptr(f32[0]), O.dptr(f32[1]), O.dptr(f64), O.dptr(B[0]), O.dptr(B[1]),
                    O.u8ptr(path), O.u8ptr(nob), O.u8ptr(stable))

    bands = [(y, y + 1) for y in range(y0, y1)]
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(bands)))) as ex:
        list(ex.map(band, bands))
    for a in (f32, f64, B, path):
        a.setflags(write=False)
    return types.SimpleNamespace(f32=f32, f64=f64, B=B, path=path, noB=np.stack([(nob & 1) != 0, (nob & 2) != 0]),
                                 stable=stable != 0)


def disparity_ranges(case, ref):
    """Column ranges for the host test, no device at hand: on the rectified pair the candidates of pixel x lie D columns to
    one side of it (to the left from view 0, to the right from view 1), clipped to the image; none for a masked pixel."""
    mask = case["views"][ref][1]
    h, w = mask.shape
    D = case["params"]["num_depth_levels"]
    x = np.arange(w, dtype=np.int32)
    lo = np.maximum(0, x - D) if ref == 0 else x
    hi = x if ref == 0 else np.minimum(w - 1, x + D)
    rng = np.empty((h, w, 2), np.int32)
    rng[..., 0], rng[..., 1] = lo[None, :], hi[None, :]
    rng[mask != 1] = (0, -1)
    return rng, D + 1
