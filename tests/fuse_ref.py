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
    |dot(n, C - P)| / (|n| |C - P|) over every orientation test made, gap_margin = min ||depth' - depth| - gap| / gap over
    every usable-neighbour test made (a neighbour inside the image that has a point)."""
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
    member_margin = orient_margin = gap_margin = math.inf
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
                nonlocal gap_margin
                if not (0 <= xx < w and 0 <= yy < h and bool(valid[yy, xx])):
                    return False
                dd = abs(float(depths[v][yy, xx]) - depth)
                gap_margin = min(gap_margin, abs(dd - gap) / gap)
                return dd <= gap

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
        n_normals=n_normals, claimed=claimed, member_margin=member_margin, orient_margin=orient_margin,
        gap_margin=gap_margin)


# ---------------------------------------------------------------- the inputs the GPU tests and the host tests share

# (case name, threshold as a multiple of the pixel footprint at the sphere's centre: depth / focal length)
FUSE_CASES = ["mvs_geodesic", "mvs_distorted", "mvs_refractive", "mvs_mixed_sizes", "mvs_scaled"]
THRESHOLD_FOOTPRINTS = 0.75
# the full rule at sizes that cross the boundaries of fuse_scan_kernel (256 threads, thread t sums a run of `per` blocks
# of 256 pixels): 304x216 is 257 blocks, per 2; 432x304 is 513 blocks, per 3; the last run is ragged in both
FUSE_SIZE_CASES = [("mvs_distorted", dict(nviews=2, w=304, h=216)), ("mvs_geodesic", dict(nviews=2, w=432, h=304))]
# srh_fuse_params.normal_depth_gap as the default gap divided by these (mvs_geodesic)
GAP_FRACTIONS = [4, 12]
# mvs_mixed_sizes with the largest view (view 0) not first: at the default size (9, 7 and 7 blocks) and at 120x80,
# 112x76, 104x80 (38, 34 and 33 blocks) in ascending size and with the largest in the middle
MIXED_ORDERS = [({}, (2, 1, 0)), ({}, (1, 2, 0)), ({}, (1, 0, 2)),
                (dict(w=120, h=80), (2, 1, 0)), (dict(w=120, h=80), (1, 0, 2))]

_inputs = {}


def case_inputs(name, **over):
    """-> dict(case, ocams, op, rgbas, masks, depths, thr): tests/cases.py's scene `name` (`over`: get_mvs's overrides, such
    as w, h, nviews) with analytic, hole-punched depth maps and a threshold of THRESHOLD_FOOTPRINTS pixel footprints.
    Computed once per process."""
    key = (name, tuple(sorted(over.items())))
    if key in _inputs:
        return _inputs[key]
    import cases
    case = cases.get_mvs(name, **over)
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
    _inputs[key] = dict(case=case, ocams=ocams, op=op, rgbas=rgbas, masks=masks, depths=depths, thr=thr)
    return _inputs[key]


_results = {}


def case_result(name, order=None, min_views=2, gap=None, **over):
    """fuse() on case_inputs(name, **over) with the views listed in `order` (default: as they are); cached."""
    I = case_inputs(name, **over)
    n = len(I["ocams"])
    order = tuple(range(n)) if order is None else tuple(order)
    key = (name, tuple(sorted(over.items())), order, min_views, gap)
    if key not in _results:
        pick = lambda a: [a[v] for v in order]
        _results[key] = fuse(pick(I["ocams"]), I["op"], pick(I["rgbas"]), pick(I["masks"]), pick(I["depths"]), I["thr"],
                             gap=gap, min_views=min_views)
    return _results[key]


# ---------------------------------------------------------------- the compaction alone: inputs with a closed-form cloud
#
# Every slot holds the SAME pinhole camera and the same smooth depth map, with its own image and its own set of holes (NaN
# depths).  A pixel's point then projects into its own pixel of every other slot (tests/test_fuse_host.py checks that with
# the oracle, with a quarter of a pixel to spare) and meets the very same bits there, so the members of a pixel are the
# slots in which it has a point, its owner is the first of them, and the whole cloud follows from the validity planes in
# numpy: no per-pixel Python.  The holes are laid out by blocks of FUSE_BLOCK pixels, the unit of fuse_scan_kernel and
# fuse_scatter_kernel, at sizes on the scan's boundaries.

FUSE_BLOCK = 256                                        # SRH_FUSE_BLOCK (test_fuse_host.py reads it from csrc/srh_internal.hpp)
COMPACTION_SIZES = [(256, 256), (257, 256), (363, 362)]  # 256 blocks, per 1 | 257 blocks, per 2 | 514 blocks, per 3, ragged
TWIN_SIZE = (257, 256)
MANY_SIZE, MANY_VIEWS = (16, 16), 64
COMPACTION_GAP = 100.0                                  # beyond any depth difference: only validity decides a tangent
COMPACTION_THR = 1e-3                                   # the members' distance is exactly 0


def scan_layout(npix):
    """-> (blocks, blocks per run of one thread of fuse_scan_kernel, runs that hold a block)."""
    nb = (npix + FUSE_BLOCK - 1) // FUSE_BLOCK
    per = (nb + FUSE_BLOCK - 1) // FUSE_BLOCK
    return nb, per, (nb + per - 1) // per


def where_in_scan(pixel, npix):
    """'block b, run t, wave k' of a pixel, for assertion messages."""
    _, per, _ = scan_layout(npix)
    b = int(pixel) // FUSE_BLOCK
    return "pixel %d: block %d, run %d, wave %d" % (pixel, b, b // per, b // per // 64)


def hole_pattern(w, h, seed, empty_wave=1):
    """(h, w) bool, True where the pixel keeps its depth.  Blocks are full, empty, half filled or nearly empty at random;
    block 0 is empty, block 1 full, block 2 half filled; the 64 runs of wave `empty_wave` of the scan are empty (None: no
    such wave); the last block, ragged where w*h is no multiple of FUSE_BLOCK, is half filled and not empty."""
    npix = w * h
    nb, per, _ = scan_layout(npix)
    rng = np.random.default_rng(seed)
    density = np.array([1.0, 0.0, 0.5, 0.02])[rng.integers(0, 4, nb)]
    r = rng.random((nb, FUSE_BLOCK))
    blocks = r < density[:, None]
    blocks[0] = False
    blocks[1] = True
    blocks[2] = r[2] < 0.5
    if empty_wave is not None:
        blocks[64 * per * empty_wave:64 * per * (empty_wave + 1)] = False
    blocks[nb - 1] = r[nb - 1] < 0.5
    blocks[nb - 1, 3] = True
    return blocks.ravel()[:npix].reshape(h, w).copy()


def block_counts(valid_flat):
    """Points per block of FUSE_BLOCK pixels (the last block padded with zeros)."""
    nb = (valid_flat.size + FUSE_BLOCK - 1) // FUSE_BLOCK
    padded = np.zeros(nb * FUSE_BLOCK, dtype=np.int64)
    padded[:valid_flat.size] = valid_flat
    return padded.reshape(nb, FUSE_BLOCK).sum(1)


_compaction = {}


def compaction_inputs(kind, w, h):
    """kind "twin": two slots, the first with hole_pattern(seed 1, the scan's wave 1 empty), the second with another image
    and hole_pattern(seed 2, no empty wave); "many": MANY_VIEWS slots without holes.  -> dict(case, ocams, op, rgbas,
    masks, depth (the shared map, no holes), valids, depths (with the holes), C); cached."""
    key = (kind, w, h)
    if key in _compaction:
        return _compaction[key]
    import cases
    from stereoreconstruction_amd import synthetic as S
    K, R, t = S.semicircle_rig(1, w, h, radius=10.0, focal=1.4 * w)[0]
    ys, xs = np.mgrid[0:h, 0:w]
    depth = 9.0 + 0.9 * np.sin(1.5 * 2 * np.pi * (xs + 0.5) / w) * np.cos(2 * np.pi * (ys + 0.5) / h)
    if kind == "twin":
        valids = [hole_pattern(w, h, 1, 1), hole_pattern(w, h, 2, None)]
    elif kind == "many":
        valids = [np.ones((h, w), dtype=bool)] * MANY_VIEWS
    else:
        raise ValueError(kind)
    n = len(valids)
    rng = np.random.default_rng(1000 * w + h + n)
    rgbas = []
    for _ in range(n):
        im = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        im[..., 3] = 255
        rgbas.append(im)
    masks = [np.ones((h, w), dtype=np.uint8) for _ in range(n)]
    views = [(rgbas[v], masks[v], (K, R, t), None, None) for v in range(n)]
    params = dict(min_depth=7.5, max_depth=10.5, num_depth_levels=24, window_radius=2, weight_kind=1, image_scale=1.0,
                  cross_check_threshold=0.25)
    case = dict(name="compaction_" + kind, kind="mvs", views=views, params=params)
    _, ocams, op = cases.oracle_inputs(case)
    assert depth.min() >= op.min_depth and depth.max() <= op.max_depth
    _compaction[key] = dict(case=case, ocams=ocams, op=op, rgbas=rgbas, masks=masks, depth=depth, valids=valids,
                            depths=[np.where(v, depth, np.nan) for v in valids], C=np.array(ocams[0].C[:]))
    return _compaction[key]


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def _norm(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def tangent_normals(pts, valid, C):
    """fuse_view_kernel's normal for every pixel of a view whose neighbours are usable exactly where they have a point:
    pts (h, w, 3), valid (h, w) bool, C the camera centre -> (normals (h, w, 3), flags (h, w) uint8, orientation margin
    over the pixels with a point).  Garbage where valid is False."""
    with np.errstate(all="ignore"):
        ok = {k: _shift(valid, dy, dx, False) for k, (dy, dx) in dict(l=(0, -1), r=(0, 1), u=(-1, 0), d=(1, 0)).items()}
        pt = {k: _shift(pts, dy, dx, np.nan) for k, (dy, dx) in dict(l=(0, -1), r=(0, 1), u=(-1, 0), d=(1, 0)).items()}

        def tangent(lo, hi):
            both, only_hi = (ok[lo] & ok[hi])[..., None], ok[hi][..., None]
            return np.where(both, pt[hi] - pt[lo], np.where(only_hi, pt[hi] - pts, pts - pt[lo])), ok[lo] | ok[hi]
        th, have_h = tangent("l", "r")
        tv, have_v = tangent("u", "d")
        cr = np.stack([th[..., 1] * tv[..., 2] - th[..., 2] * tv[..., 1], th[..., 2] * tv[..., 0] - th[..., 0] * tv[..., 2],
                       th[..., 0] * tv[..., 1] - th[..., 1] * tv[..., 0]], axis=-1)
        ln = _norm(cr)
        has = have_h & have_v & np.isfinite(ln) & (ln > 0)
        nv = cr / ln[..., None]
        to_cam = C[None, None, :] - pts
        d = (nv[..., 0] * to_cam[..., 0] + nv[..., 1] * to_cam[..., 1]) + nv[..., 2] * to_cam[..., 2]
        margin = np.abs(d) / (_norm(nv) * _norm(to_cam))
        nv = np.where((d < 0)[..., None], -nv, nv)
        nv = np.where(has[..., None], nv, to_cam / _norm(to_cam)[..., None])
    sel = has & valid
    return nv, has.astype(np.uint8), (float(margin[sel].min()) if sel.any() else math.inf)


def same_camera_cloud(pts, valids, rgbas, C, min_views):
    """The fused cloud of slots that share camera and depth map (see above), in numpy: pts (h, w, 3) the point of every
    pixel, valids / rgbas per slot.  -> the dict of fuse(), without `claimed` and the member and gap margins."""
    n = len(valids)
    V = np.stack([v.ravel() for v in valids])
    P = pts.reshape(-1, 3)
    m = V.sum(0)
    first = V.argmax(0)
    acc = np.zeros_like(P)
    started = np.zeros(P.shape[0], dtype=bool)
    col = np.zeros((P.shape[0], 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        for u in range(n):
            acc = np.where(V[u][:, None], np.where(started[:, None], acc + P, P), acc)
            started |= V[u]
            col += V[u][:, None] * rgbas[u].reshape(-1, 4)[:, :3].astype(np.int64)
        mean = acc / m[:, None].astype(np.float64)
        mm = np.maximum(m, 1)[:, None]
        colour = ((2 * col + mm) // (2 * mm)).astype(np.uint8)
    out = {k: [] for k in ("xyz", "normals", "rgb", "nviews", "flags", "src")}
    orient_margin = math.inf
    for v in range(n):
        idx = np.flatnonzero(V[v] & (first == v) & (m >= min_views))
        if idx.size == 0 and not V[v].any():
            continue
        nrm, flg, margin = tangent_normals(pts, valids[v], C)
        orient_margin = min(orient_margin, margin)
        out["xyz"].append(mean[idx])
        out["normals"].append(nrm.reshape(-1, 3)[idx])
        out["rgb"].append(colour[idx])
        out["nviews"].append(m[idx].astype(np.uint8))
        out["flags"].append(flg.ravel()[idx])
        out["src"].append(np.stack([np.full(idx.size, v), idx], axis=1).astype(np.int32))
    empty = dict(xyz=np.zeros((0, 3)), normals=np.zeros((0, 3)), rgb=np.zeros((0, 3), np.uint8), nviews=np.zeros(0, np.uint8),
                 flags=np.zeros(0, np.uint8), src=np.zeros((0, 2), np.int32))
    out = {k: (np.concatenate(a) if a else empty[k]) for k, a in out.items()}
    supported = m >= min_views
    out.update(n_points=int(out["src"].shape[0]), n_candidates=int(V.sum()), n_claimed=int((m[supported] - 1).sum()),
               n_unsupported=int(m[~supported].sum()), n_normals=int(out["flags"].sum()), orient_margin=orient_margin)
    return out


# ---------------------------------------------------------------- the comparison of the GPU tests

COUNTERS = ("n_points", "n_candidates", "n_claimed", "n_unsupported", "n_normals")


def _first_difference(got, want, bad, npix):
    """Where the clouds first differ: the output position and, from the source the restatement expects there, the block
    of SRH_FUSE_BLOCK pixels, the scan's run and its wave (npix: the pixels of every list entry, or None)."""
    bad = bad.reshape(bad.shape[0], -1).any(axis=1)
    k = int(np.flatnonzero(bad)[0])
    v, i = (int(q) for q in want["src"][k])
    msg = "first at output position %d of %d (%d positions differ): expected source entry %d" % (k, bad.size, int(bad.sum()), v)
    msg += ", " + (where_in_scan(i, npix[v]) if npix is not None else "pixel %d" % i)
    return msg + "; the device has source (%d, %d) there" % tuple(int(q) for q in got["src"][k])


def assert_equal(got, want, tag="", npix=None):
    for k in COUNTERS:
        assert got[k] == want[k], "%s %s: %d != %d" % (tag, k, got[k], want[k])
    assert got["normals"].shape == want["normals"].shape
    for k in ("src", "nviews", "flags", "rgb"):
        assert got[k].shape == want[k].shape, "%s %s" % (tag, k)
        bad = got[k] != want[k]
        assert not bad.any(), "%s %s: %s" % (tag, k, _first_difference(got, want, bad, npix))
    bad = got["xyz"].view(np.uint64) != want["xyz"].view(np.uint64)
    assert not bad.any(), "%s xyz bits: %s" % (tag, _first_difference(got, want, bad, npix))
    if want["n_points"]:
        bad = ~(np.abs(got["normals"] - want["normals"]) <= 1e-12)
        assert not bad.any(), "%s normals: %s" % (tag, _first_difference(got, want, bad, npix))
