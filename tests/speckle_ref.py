"""The speckle filter's reference (srh_view_filter_speckles; include/stereo_recon_hip.h states the definition): plain
NumPy / Python union-find.  `components` is the vectorised form the large maps need (hook every joined pair's larger root
under the smaller, jump pointers, repeat); `components_slow` is the textbook loop over the pixels, which the CPU suite
holds the fast form against.  Also the maps the CPU and the GPU tests share, and a ctypes driver of
csrc/srh_speckle.hpp compiled for the host (tests/speckle_host.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from filter_ref import same_bits  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereoreconstruction_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "speckle_host.cpp")
inf, nan = np.inf, np.nan
COUNTERS = ("valid", "components", "removed_components", "removed_pixels", "largest")


def default_max_diff(p, steps=2.0):
    """max_diff <= 0: two depth steps of p -- the header's expression, evaluated as it is written."""
    return float(steps) * ((p.max_depth - p.min_depth) / float(p.num_depth_levels - 1))


def valid_pixels(depth, mask):
    d = np.asarray(depth, np.float64)
    white = np.ones(d.shape, bool) if mask is None else (np.asarray(mask) == 1)
    with np.errstate(invalid="ignore"):
        return white & np.isfinite(d) & (d > 0)


def _joins(d, valid, max_diff):
    """(a, b): linear indices of the joined pairs, horizontal ones then vertical ones"""
    h, w = d.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    with np.errstate(invalid="ignore"):
        hj = valid[:, :-1] & valid[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= max_diff)
        vj = valid[:-1] & valid[1:] & (np.abs(d[:-1] - d[1:]) <= max_diff)
    return (np.concatenate([idx[:, :-1][hj], idx[:-1][vj]]), np.concatenate([idx[:, 1:][hj], idx[1:][vj]]))


def components(depth, mask, max_diff):
    """(labels (h, w) int32: smallest linear index of the pixel's component, -1 = not valid; sizes (h*w,) int64: member
    count at every label)"""
    d = np.ascontiguousarray(depth, np.float64)
    h, w = d.shape
    valid = valid_pixels(d, mask)
    a, b = _joins(d, valid, float(max_diff))
    lab = np.arange(h * w, dtype=np.int64)
    while a.size:
        la, lb = lab[a], lab[b]
        open_ = la != lb
        if not open_.any():
            break
        a, b, la, lb = a[open_], b[open_], la[open_], lb[open_]       # (a pair inside one tree stays inside it)
        np.minimum.at(lab, np.maximum(la, lb), np.minimum(la, lb))     # roots only: lab[a] is a root after the jumps
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    labels = np.where(valid.reshape(-1), lab, -1).astype(np.int32).reshape(h, w)
    sizes = np.bincount(lab[valid.reshape(-1)], minlength=h * w).astype(np.int64)
    return labels, sizes


def components_slow(depth, mask, max_diff):
    """The same by the textbook: one pass over the pixels, union by smaller index, path halving."""
    d = np.ascontiguousarray(depth, np.float64)
    h, w = d.shape
    valid = valid_pixels(d, mask)
    parent = list(range(h * w))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def union(i, j):
        i, j = find(i), find(j)
        if i != j:
            parent[max(i, j)] = min(i, j)

    for y in range(h):
        for x in range(w):
            if not valid[y, x]:
                continue
            if x + 1 < w and valid[y, x + 1] and abs(float(d[y, x]) - float(d[y, x + 1])) <= max_diff:
                union(y * w + x, y * w + x + 1)
            if y + 1 < h and valid[y + 1, x] and abs(float(d[y, x]) - float(d[y + 1, x])) <= max_diff:
                union(y * w + x, (y + 1) * w + x)
    labels = np.full(h * w, -1, np.int32)
    sizes = np.zeros(h * w, np.int64)
    for i in np.flatnonzero(valid.reshape(-1)):
        r = find(int(i))
        labels[i] = r
        sizes[r] += 1
    return labels.reshape(h, w), sizes


def apply(depth, labels, sizes, min_size, to_nan=False):
    """The removal, from the labelling: (filtered map, info)"""
    d = np.array(depth, np.float64, copy=True)
    flat = labels.reshape(-1)
    valid = flat >= 0
    size_of = np.where(valid, sizes[np.maximum(flat, 0)], 0)
    removed = valid & (size_of < min_size)
    d.reshape(-1)[removed] = nan if to_nan else inf
    roots = valid & (flat == np.arange(flat.size))
    info = dict(valid=int(valid.sum()), components=int(roots.sum()), removed_components=int((roots & removed).sum()),
                removed_pixels=int(removed.sum()), largest=int(sizes.max()) if valid.any() else 0)
    return d, info


def filter_map(depth, mask, min_size, max_diff, to_nan=False):
    """srh_view_filter_speckles on one map -> (filtered map, labels, info)"""
    labels, sizes = components(depth, mask, max_diff)
    out, info = apply(depth, labels, sizes, min_size, to_nan)
    return out, labels, info


# ---------------------------------------------------------------- the maps the CPU and the GPU tests share

def serpentine(w, h):
    """(depth, size): one path, one pixel wide: every even row whole, joined to the next even row at alternating ends"""
    d = np.full((h, w), inf)
    d[0::2] = 40.0
    for k, y in enumerate(range(1, h - 1, 2)):
        d[y, w - 1 if k % 2 == 0 else 0] = 40.0
    return d, int(np.isfinite(d).sum())


def comb(w, h):
    """vertical teeth two pixels apart, joined only by the bottom row"""
    d = np.full((h, w), inf)
    d[:, 0::2] = 40.0
    d[h - 1] = 40.0
    return d


def checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, 40.0, inf)


def staircase(w, h):
    return np.tile(30.0 + 0.25 * np.arange(w), (h, 1))


CORNERS = [(x, y) for y in (15, 31, 47, 63) for x in (15, 31, 47, 63, 79, 95, 111, 127)]


def corner_straddlers(w, h):
    """2x2 islands on every crossing of tile borders for tiles of 16, 32 and 64; everything else invalid"""
    d = np.full((h, w), nan)
    for x, y in CORNERS:
        d[y:y + 2, x:x + 2] = 40.0
    return d


def ragged_mask(w, h, rng):
    """the ragged left edge + 2 % holes of test_gpu_filter._synthetic"""
    x = np.arange(w)[None, :]
    mask = (x >= (w // 16 + (np.arange(h)[:, None] * 7919 % 37))).astype(np.uint8)
    mask[rng.random((h, w)) < 0.02] = 0
    return mask


RANDOM_MAX_DIFF = 0.5


def random_map(w, h, seed):
    """(mask, depth): a few plateaus, a per-pixel jitter that stays below max_diff between most neighbours and exceeds it
    between some, about 30 % of the pixels invalid: +INF, NaN, -1 and mask 0"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    plateaus = np.array([35.0, 40.0, 45.5, 52.25, 60.0, 71.0])
    depth = plateaus[((x // 37) + (y // 23) * 3) % len(plateaus)] + 0.0
    jitter = np.where(rng.random((h, w)) < 0.8, rng.uniform(-0.2, 0.2, (h, w)), rng.uniform(-0.9, 0.9, (h, w)))
    depth += jitter
    kind = rng.random((h, w))
    depth[kind < 0.08] = inf
    depth[(kind >= 0.08) & (kind < 0.16)] = nan
    depth[(kind >= 0.16) & (kind < 0.22)] = -1.0
    mask = ragged_mask(w, h, rng)
    return mask, depth


# ---------------------------------------------------------------- csrc/srh_speckle.hpp on the host

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    out = os.path.join(tempfile.mkdtemp(prefix="speckle_host_"), "libspeckle_host.so")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, SRC, "-o", out])
    L = C.CDLL(out)
    L.sp_label.argtypes = [C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double, C.c_int,
                           C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sp_label.restype = None
    L.sp_depth_steps.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double]
    L.sp_depth_steps.restype = C.c_double
    _lib = L
    return L


def lib_components(depth, mask, max_diff, order=0):
    """The header's valid / joined / unite / find driven sequentially over the map (order 1: the pairs back to front)
    -> (labels, sizes) as `components` gives them"""
    d = np.ascontiguousarray(depth, np.float64)
    h, w = d.shape
    m = np.ones((h, w), np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8)
    labels = np.empty((h, w), np.int32)
    sizes = np.empty(h * w, np.int32)
    lib().sp_label(m.ctypes.data_as(C.POINTER(C.c_uint8)), d.ctypes.data_as(C.POINTER(C.c_double)), w, h, float(max_diff),
                   order, labels.ctypes.data_as(C.POINTER(C.c_int32)), sizes.ctypes.data_as(C.POINTER(C.c_int32)))
    return labels, sizes.astype(np.int64)
