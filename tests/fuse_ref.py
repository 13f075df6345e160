"""CPU restatement of depth-map fusion (srh_mvs_fuse; include/stereo_recon_hip.h).

Geometry comes from the oracle (oracle_ffi: sro_back_project for a pixel's point, sro_project for the projection into
another view, sro_unproject for the analytic depth maps of the tests); everything else -- members, support, the mean,
the colour, claims, normals, the ordered output -- is restated here in plain Python floats (IEEE double, no contraction),
the norm in the device's operation order sqrt((x*x + y*y) + z*z).

TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

import oracle_ffi as O


def norm3(a):
    return math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def point_map(ocam, op, depth, mask):
    """-> (pts (h, w, 3) float64, NaN where there is no point; valid (h, w) bool): point_cloud_kernel's construction."""
    h, w = depth.shape
    pts = np.full((h, w, 3), np.nan)
    valid = np.zeros((h, w), dtype=bool)
    out3 = np.zeros(3)
    L = O.lib()
    for y, x in np.argwhere((mask == 1) & np.isfinite(depth)):
        if L.sro_back_project(ocam, op, int(x), int(y), float(depth[y, x]), O.dptr(out3)):
            pts[y, x] = out3
            valid[y, x] = True
    return pts, valid


def sphere_depths(ocams, op, shapes, sphere_radius=2.0):
    """Analytic depth maps: every pixel's oracle ray (the camera's own: distortion, refraction, scale) cut with the
    sphere |X| = sphere_radius of tests/cases.py's MVS scenes; the depth is the plane depth pointFromDepth inverts
    (along the principal direction from the camera centre).  NaN where the ray misses."""
    L = O.lib()
    out = []
    src, dr = np.zeros(3), np.zeros(3)
    for cam, (h, w) in zip(ocams, shapes):
        D = np.full((h, w), np.nan)
        C = np.array(cam.C[:])
        pd = np.array(cam.pdir[:])
        for y in range(h):
            for x in range(w):
                L.sro_unproject(cam, (x + 0.5) / op.image_scale, (y + 0.5) / op.image_scale, O.dptr(src), O.dptr(dr))
                b = float(src @ dr)
                disc = b * b - (float(src @ src) - sphere_radius ** 2)
                if disc <= 0:
                    continue
                t = -b - math.sqrt(disc)
                if t <= 0:
                    continue
                D[y, x] = float(pd @ (src + t * dr - C)) / float(pd @ pd)
        out.append(D)
    return out


def punch_holes(depths, masks, step=9):
    """Copies of the depth maps with every kind of hole on a lattice: around a centre every `step` pixels the four
    neighbours become NaN, +INF, -1 ("no peak": finite, no point) and NaN, so that the centre keeps its point and has no
    tangent; and copies of the masks with one pixel per lattice cell masked out.  Deterministic."""
    outd, outm = [], []
    for v, (D, M) in enumerate(zip(depths, masks)):
        D = D.copy()
        M = M.copy()
        h, w = D.shape
        for cy in range(3 + v % 3, h - 1, step):
            for cx in range(4 + v % 2, w - 1, step):
                D[cy, cx - 1] = np.nan
                D[cy, cx + 1] = np.inf
                D[cy - 1, cx] = -1.0
                D[cy + 1, cx] = np.nan
                if cy + 3 < h and cx + 3 < w:
                    M[cy + 3, cx + 3] = 0
        outd.append(D)
        outm.append(M)
    return outd, outm


def default_gap(op):
    return 2 * (op.max_depth - op.min_depth) / (op.num_depth_levels - 1)


def fuse(ocams, op, rgbas, masks, depths, thr, gap=None, min_views=2, maps=None):
    """The rule of srh_mvs_fuse over the views in the order given (the slot list).  -> dict with the output arrays (xyz,
    normals, rgb, nviews, flags, src), the info counters, `claimed` (list of (h, w) bool), and the margins the tests
    ask about: member_margin = min |nrm - thr| / thr over every member test made, orient_margin = min
    |dot(n, C - P)| / (|n| |C - P|) over every orientation test made."""
    n = len(ocams)
    if gap is None:
        gap = default_gap(op)
    if maps is None:
        maps = [point_map(ocams[v], op, depths[v], masks[v]) for v in range(n)]
    L = O.lib()
    s = op.image_scale
    claimed = [np.zeros(m[1].shape, dtype=bool) for m in maps]
    xyz, nrm, rgb, nvw, flg, src = [], [], [], [], [], []
    n_claimed = n_unsup = n_normals = 0
    member_margin = orient_margin = math.inf
    q = np.zeros(3)
    for v in range(n):
        pts, valid = maps[v]
        h, w = valid.shape
        C = [float(c) for c in ocams[v].C[:]]
        for y, x in np.argwhere(valid):
            y, x = int(y), int(x)
            if claimed[v][y, x]:
                n_claimed += 1
                continue
            P1 = [float(c) for c in pts[y, x]]
            members = []                                   # (u, y2, x2, point) in ascending u
            for u in range(n):
                if u == v:
                    members.append((u, y, x, P1))
                    continue
                q[:] = P1
                if not L.sro_project(ocams[u], O.dptr(q)):
                    continue
                x2, y2 = float(q[0]) * s, float(q[1]) * s
                hu, wu = maps[u][1].shape
                if not (x2 >= 0 and y2 >= 0 and x2 < wu and y2 < hu):
                    continue
                jx, jy = int(x2), int(y2)
                if not maps[u][1][jy, jx]:
                    continue
                P2 = [float(c) for c in maps[u][0][jy, jx]]
                d = norm3([P1[0] - P2[0], P1[1] - P2[1], P1[2] - P2[2]])
                if math.isfinite(d):
                    member_margin = min(member_margin, abs(d - thr) / thr)
                if math.isfinite(d) and d < thr:
                    members.append((u, jy, jx, P2))
            m = len(members)
            if m < min_views:
                n_unsup += 1
                continue
            acc = list(members[0][3])
            for (_, _, _, Pm) in members[1:]:
                acc = [acc[0] + Pm[0], acc[1] + Pm[1], acc[2] + Pm[2]]
            xyz.append([acc[0] / float(m), acc[1] / float(m), acc[2] / float(m)])
            col = [0, 0, 0]
            for (u, yy, xx, _) in members:
                for k in range(3):
                    col[k] += int(rgbas[u][yy, xx, k])
                if u > v:
                    claimed[u][yy, xx] = True
            rgb.append([(2 * c + m) // (2 * m) for c in col])
            nvw.append(m)
            src.append([v, y * w + x])
            # the normal, from v's own point map
            depth = float(depths[v][y, x])

            def usable(yy, xx):
                return 0 <= xx < w and 0 <= yy < h and bool(valid[yy, xx]) and abs(float(depths[v][yy, xx]) - depth) <= gap

            def tangent(lo, hi):
                lo_ok, hi_ok = usable(*lo), usable(*hi)
                pl = [float(c) for c in pts[lo]] if lo_ok else None
                ph = [float(c) for c in pts[hi]] if hi_ok else None
                if lo_ok and hi_ok:
                    return [ph[k] - pl[k] for k in range(3)]
                if hi_ok:
                    return [ph[k] - P1[k] for k in range(3)]
                if lo_ok:
                    return [P1[k] - pl[k] for k in range(3)]
                return None

            th = tangent((y, x - 1), (y, x + 1))
            tv = tangent((y - 1, x), (y + 1, x))
            to_cam = [C[k] - P1[k] for k in range(3)]
            nv, has = None, 0
            if th is not None and tv is not None:
                cr = [th[1] * tv[2] - th[2] * tv[1], th[2] * tv[0] - th[0] * tv[2], th[0] * tv[1] - th[1] * tv[0]]
                ln = norm3(cr)
                if math.isfinite(ln) and ln > 0:
                    nv = [cr[0] / ln, cr[1] / ln, cr[2] / ln]
                    d = dot3(nv, to_cam)
                    orient_margin = min(orient_margin, abs(d) / (norm3(nv) * norm3(to_cam)))
                    if d < 0:
                        nv = [-nv[0], -nv[1], -nv[2]]
                    has = 1
            if not has:
                ln = norm3(to_cam)
                nv = [to_cam[0] / ln, to_cam[1] / ln, to_cam[2] / ln]
            nrm.append(nv)
            flg.append(has)
            n_normals += has
    k = len(xyz)
    return dict(
        xyz=np.array(xyz, dtype=np.float64).reshape(k, 3), normals=np.array(nrm, dtype=np.float64).reshape(k, 3),
        rgb=np.array(rgb, dtype=np.uint8).reshape(k, 3), nviews=np.array(nvw, dtype=np.uint8),
        flags=np.array(flg, dtype=np.uint8), src=np.array(src, dtype=np.int32).reshape(k, 2),
        n_points=k, n_candidates=int(sum(int(m[1].sum()) for m in maps)), n_claimed=n_claimed, n_unsupported=n_unsup,
        n_normals=n_normals, claimed=claimed, member_margin=member_margin, orient_margin=orient_margin)


# ---------------------------------------------------------------- the inputs the GPU tests and the host tests share

# (case name, threshold as a multiple of the pixel footprint at the sphere's centre: depth / focal length)
FUSE_CASES = ["mvs_geodesic", "mvs_distorted", "mvs_refractive", "mvs_mixed_sizes", "mvs_scaled"]
THRESHOLD_FOOTPRINTS = 0.75

_inputs = {}


def case_inputs(name):
    """-> dict(case, ocams, op, rgbas, masks, depths, thr): tests/cases.py's scene `name` with analytic, hole-punched depth
    maps and a threshold of THRESHOLD_FOOTPRINTS pixel footprints.  Computed once per process."""
    if name in _inputs:
        return _inputs[name]
    import cases
    case = cases.get_mvs(name)
    imgs, ocams, op = cases.oracle_inputs(case)
    rgbas = [v[0] for v in case["views"]]
    masks = [v[1] for v in case["views"]]
    depths = sphere_depths(ocams, op, [m.shape for m in masks])
    depths, masks = punch_holes(depths, masks)
    views = [(rg, mk) + tuple(v[2:]) for rg, mk, v in zip(rgbas, masks, case["views"])]
    case = dict(case, views=views)
    # footprint of a pixel of the images handed over, at the distance of the sphere's centre
    focal = float(case["views"][0][2][0][0, 0]) * op.image_scale
    thr = THRESHOLD_FOOTPRINTS * 10.0 / focal
    _inputs[name] = dict(case=case, ocams=ocams, op=op, rgbas=rgbas, masks=masks, depths=depths, thr=thr)
    return _inputs[name]


_results = {}


def case_result(name, order=None, min_views=2):
    """fuse() on case_inputs(name) with the views listed in `order` (default: as they are); cached."""
    I = case_inputs(name)
    n = len(I["ocams"])
    order = tuple(range(n)) if order is None else tuple(order)
    key = (name, order, min_views)
    if key not in _results:
        pick = lambda a: [a[v] for v in order]
        _results[key] = fuse(pick(I["ocams"]), I["op"], pick(I["rgbas"]), pick(I["masks"]), pick(I["depths"]), I["thr"],
                             min_views=min_views)
    return _results[key]
