"""The CPU restatement of MultiViewStereo's semi-global aggregation over the top-K peak labels (include/stereo_recon_hip.h,
"MultiViewStereo, semi-global aggregation"; csrc/srh_mvs_sgm.hip), in two forms:

  aggregate          numpy, vectorised over the path lines of a direction: the minimum over k is taken in ascending k with
                     np.where(M > c, c, M), the label with np.argmin (the lowest index among equal minima);
  aggregate_loops    plain Python, pixel by pixel, label pair by label pair, for tiny grids.

Labels 0 .. K-1 are a pixel's peaks (cost, depth), K is "unknown".  Every + and - is one IEEE double operation; the
pairwise term between two peaks is 2.0*fabs(zq - zp)/(zq + zp): one subtraction, one addition, one product, one division."""
import numpy as np

DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
DEFAULTS = dict(beta=1.0, lam=1.0, phi_u=0.5, psi_u=0.002, mask=0xFF)


def popcount(mask):
    return bin(mask).count("1")


def data_costs(peaks, beta=1.0, lam=1.0, phi_u=0.5):
    """D (h, w, K+1) with numpy's exp (the device's own exp may differ in the last places)"""
    h, w, K, _ = peaks.shape
    D = np.empty((h, w, K + 1))
    D[..., :K] = np.where(peaks[..., 1] < 0, lam, lam * np.exp(-beta * peaks[..., 0]))
    D[..., K] = phi_u
    return D


def smooth(zq, k, zp, d, K, psi_u):
    """V(q, k; p, d), scalar: zq / zp the depth of that peak label (ignored for label K)"""
    if k == K and d == K:
        return 0.0
    if k == K or d == K:
        return psi_u
    if zq < 0 or zp < 0:
        return 2 * psi_u
    return 2.0 * abs(zq - zp) / (zq + zp)


def smooth_matrix(zq, zp, psi_u):
    """zq, zp (N, K) peak depths of N edges -> V (N, K+1 [label k of q], K+1 [label d of p])"""
    N, K = zq.shape
    V = np.empty((N, K + 1, K + 1))
    a, b = zq[:, :, None], zp[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = 2.0 * np.abs(a - b) / (a + b)
    V[:, :K, :K] = np.where((a < 0) | (b < 0), 2 * psi_u, quot)
    V[:, K, :] = psi_u
    V[:, :, K] = psi_u
    V[:, K, K] = 0.0
    return V


def message(prev, zq, zp, psi_u):
    """prev (N, L), zq / zp (N, K) -> (M (N, L), g (N, 1)); minima in ascending k"""
    L = prev.shape[1]
    V = smooth_matrix(zq, zp, psi_u)
    M = prev[:, 0, None] + V[:, 0, :]
    g = prev[:, 0, None]
    for k in range(1, L):
        c = prev[:, k, None] + V[:, k, :]
        M = np.where(M > c, c, M)
        pk = prev[:, k, None]
        g = np.where(g > pk, pk, g)
    return M, g


def path(D, z, k, psi_u):
    """L_k of the data costs D (h, w, L) with the peak depths z (h, w, K)"""
    h, w, L = D.shape
    dx, dy = DIRS[k]
    out = np.empty_like(D)
    if dy == 0:
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for x in xs:
            q = x - dx
            if q < 0 or q >= w:
                out[:, x] = D[:, x]
            else:
                M, g = message(out[:, q], z[:, q], z[:, x], psi_u)
                out[:, x] = D[:, x] + (M - g)
        return out
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    for y in ys:
        q = y - dy
        out[y] = D[y]
        if q < 0 or q >= h:
            continue
        x = np.arange(w)
        has = (x - dx >= 0) & (x - dx < w)
        if not has.any():
            continue
        M, g = message(out[q, x[has] - dx], z[q, x[has] - dx], z[y, has], psi_u)
        out[y, has] = D[y, has] + (M - g)
    return out


def path_loops(D, z, k, psi_u):
    """L_k, scalar: the definition as written"""
    h, w, L = D.shape
    K = L - 1
    dx, dy = DIRS[k]
    out = np.empty_like(D)
    ys = range(h) if dy >= 0 else range(h - 1, -1, -1)
    xs = list(range(w) if dx >= 0 else range(w - 1, -1, -1))
    for y in ys:
        for x in xs:
            qx, qy = x - dx, y - dy
            if qx < 0 or qx >= w or qy < 0 or qy >= h:
                out[y, x] = D[y, x]
                continue
            prev = [float(v) for v in out[qy, qx]]
            zq = [float(v) for v in z[qy, qx]] + [0.0]
            zp = [float(v) for v in z[y, x]] + [0.0]
            g = prev[0]
            for v in prev:
                g = v if g > v else g
            for d in range(L):
                best = None
                for kk in range(L):
                    t = prev[kk] + smooth(zq[kk], kk, zp[d], d, K, psi_u)
                    best = t if best is None or best > t else best
                out[y, x, d] = float(D[y, x, d]) + (best - g)
    return out


def energy(D, z, labels, psi_u):
    """totalEnergy() of a labelling under the MRF branch's energy, the terms added one after the other in the oracle's order
    (per pixel: its data cost, its edge to x+1, its edge to y+1)"""
    h, w, L = D.shape
    K = L - 1
    yy, xx = np.mgrid[0:h, 0:w]
    zl = np.where(labels == K, 0.0, np.take_along_axis(np.concatenate([z, np.zeros((h, w, 1))], axis=2), labels[..., None], axis=2)[..., 0])

    def pair(la, za, lb, zb):
        with np.errstate(divide="ignore", invalid="ignore"):
            quot = 2.0 * np.abs(za - zb) / (za + zb)
        v = np.where((za < 0) | (zb < 0), 2 * psi_u, quot)
        v = np.where((la == K) | (lb == K), psi_u, v)
        return np.where((la == K) & (lb == K), 0.0, v)

    terms = np.zeros((h, w, 3))
    terms[..., 0] = D[yy, xx, labels]
    if w > 1:
        terms[:, :-1, 1] = pair(labels[:, :-1], zl[:, :-1], labels[:, 1:], zl[:, 1:])
    if h > 1:
        terms[:-1, :, 2] = pair(labels[:-1], zl[:-1], labels[1:], zl[1:])
    return float(np.cumsum(terms.ravel())[-1])                           # (x + 0.0 is x: the missing edges change no bit)


def depth_rule(z, labels, view_mask, depth):
    """mrf_depth_kernel's: where the mask is WHITE the chosen peak's depth if it is > 0, else +INF; untouched elsewhere"""
    h, w, K = z.shape
    zl = np.take_along_axis(np.concatenate([z, np.full((h, w, 1), np.inf)], axis=2), labels[..., None], axis=2)[..., 0]
    d = np.where(zl > 0, zl, np.inf)
    out = np.array(depth, dtype=np.float64, copy=True) if depth is not None else np.full((h, w), np.inf)
    if view_mask is None:
        return d
    return np.where(view_mask == 1, d, out)


def finish(D, z, paths, psi_u, mask, view_mask=None, depth=None):
    S = None
    for k in range(8):
        if mask >> k & 1:
            S = paths[k].copy() if S is None else S + paths[k]
    labels = np.argmin(S, axis=2).astype(np.int32)                      # the lowest index among equal minima
    return dict(S=S, labels=labels, paths=paths, depth=depth_rule(z, labels, view_mask, depth), energy=energy(D, z, labels, psi_u))


def aggregate(peaks, D=None, beta=1.0, lam=1.0, phi_u=0.5, psi_u=0.002, mask=0xFF, view_mask=None, depth=None, form=path):
    """peaks (h, w, K, 2) -> dict(S, labels, paths {k: L_k}, depth, energy); D: the data costs to use (default: numpy's exp)"""
    assert 0 < mask <= 0xFF
    peaks = np.ascontiguousarray(peaks, np.float64)
    z = np.ascontiguousarray(peaks[..., 1])
    D = data_costs(peaks, beta, lam, phi_u) if D is None else np.ascontiguousarray(D, np.float64)
    paths = {k: form(D, z, k, psi_u) for k in range(8) if mask >> k & 1}
    return finish(D, z, paths, psi_u, mask, view_mask, depth)


def aggregate_loops(peaks, **kw):
    return aggregate(peaks, form=path_loops, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
