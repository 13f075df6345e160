"""The CPU restatement of TwoViewStereo's semi-global aggregation (include/stereo_recon_hip.h, "semi-global aggregation";
csrc/srh_twoview_sgm.hip), in two forms:

  aggregate          numpy, the WINDOW form of the message, vectorised over the path lines of a direction;
  aggregate_direct   plain Python, the DIRECT O(L^2) form  min_k (prev[k] + lambda*min(|d - k|, smooth_max)),  for tiny
                     volumes.

Every + and - is one IEEE double operation, lambda*|j| and lambda*smooth_max one product each; a minimum is taken with
">" (of two equal finite numbers either is the same bits).  depthFromLabel and the energy are those of the MRF stage's
restatement (tests/twoview_mrf_restatement.cpp through twoview_mrf_ref)."""
import numpy as np

import twoview_mrf_ref as R

DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
DEFAULTS = dict(lam=0.25, smax=2.0, mask=0xFF)


def popcount(mask):
    return bin(mask).count("1")


def _min(a, b):
    return np.where(a > b, b, a)


def message(prev, lam, smax):
    """prev (N, L) -> (M (N, L), g (N, 1)): the window form"""
    L = prev.shape[1]
    g = prev.min(axis=1, keepdims=True)
    m = prev + lam * 0.0
    for j in (1, 2, 3):
        if not j < smax:
            break
        c = lam * float(j)
        if j < L:
            t = np.full_like(prev, np.inf)
            t[:, j:] = prev[:, :L - j] + c
            m = _min(m, t)
            t = np.full_like(prev, np.inf)
            t[:, :L - j] = prev[:, j:] + c
            m = _min(m, t)
    gm = g + lam * smax
    return _min(m, gm), g


def path(C, k, lam, smax):
    """L_k of the volume C (h, w, L)"""
    h, w, L = C.shape
    dx, dy = DIRS[k]
    out = np.empty_like(C)
    if dy == 0:
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for x in xs:
            q = x - dx
            if q < 0 or q >= w:
                out[:, x] = C[:, x]
            else:
                M, g = message(out[:, q], lam, smax)
                out[:, x] = C[:, x] + (M - g)
        return out
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    for y in ys:
        q = y - dy
        out[y] = C[y]
        if q < 0 or q >= h:
            continue
        x = np.arange(w)
        has = (x - dx >= 0) & (x - dx < w)
        if not has.any():
            continue
        M, g = message(out[q, x[has] - dx], lam, smax)
        out[y, has] = C[y, has] + (M - g)
    return out


def path_direct(C, k, lam, smax):
    """L_k by the direct form, scalar"""
    h, w, L = C.shape
    dx, dy = DIRS[k]
    out = np.empty_like(C)
    ys = range(h) if dy >= 0 else range(h - 1, -1, -1)
    xs = list(range(w) if dx >= 0 else range(w - 1, -1, -1))
    for y in ys:
        for x in xs:
            qx, qy = x - dx, y - dy
            if qx < 0 or qx >= w or qy < 0 or qy >= h:
                out[y, x] = C[y, x]
                continue
            prev = [float(v) for v in out[qy, qx]]
            g = prev[0]
            for v in prev:
                g = v if g > v else g
            for d in range(L):
                best = None
                for kk in range(L):
                    dist = float(abs(d - kk))
                    t = prev[kk] + lam * (dist if dist < smax else smax)
                    best = t if best is None or best > t else best
                out[y, x, d] = float(C[y, x, d]) + (best - g)
    return out


def depth_table(L, min_depth, max_depth):
    return np.array([R.depth_from_label(d, L, min_depth, max_depth) for d in range(L)])


def _finish(C, paths, lam, smax, mask, view_mask, min_depth, max_depth):
    S = None
    for k in range(8):
        if mask >> k & 1:
            S = paths[k].copy() if S is None else S + paths[k]
    labels = np.argmin(S, axis=2).astype(np.int32)                      # the lowest index among equal minima
    depth = depth_table(C.shape[2], min_depth, max_depth)[labels]
    if view_mask is not None:
        depth = np.where(view_mask == 1, depth, np.nan)
    return dict(S=S, labels=labels, paths=paths, depth=depth, energy=R.energy(C, labels, lam, smax))


def aggregate(C, lam=0.25, smax=2.0, mask=0xFF, view_mask=None, min_depth=1.0, max_depth=2.0, form=path):
    """C (h, w, L) float64 -> dict(S, labels, paths {k: L_k}, depth, energy)"""
    assert 0 < mask <= 0xFF
    C = np.ascontiguousarray(C, np.float64)
    paths = {k: form(C, k, lam, smax) for k in range(8) if mask >> k & 1}
    return _finish(C, paths, lam, smax, mask, view_mask, min_depth, max_depth)


def aggregate_direct(C, lam=0.25, smax=2.0, mask=0xFF, **kw):
    return aggregate(C, lam, smax, mask, form=path_direct, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
